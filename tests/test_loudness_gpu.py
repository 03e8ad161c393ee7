"""LoudnessBatch on the GPU against the numpy restatement of its definition (tests/loudness_helpers.py): the np.longdouble
sequential recurrence is the reference of every bound, none is measured against the code under test.

Bars (the issue's): energies |e - e_ref| <= 1e-10 * 4800 * max|x|^2 per stream; loudness values within 1e-6 LU wherever the
block is above -70 LUFS, below it only the gate decision; sample peak exact; true peak within 1e-12 * max|x|.  Every case asserts
on the reference side that no block lies within 1e-6 LU of a threshold, so no comparison is skipped silently.  One recording
[9, 33 * 4800 + 7] is filtered once in np.longdouble; the recurrence is causal, so every shorter T is a prefix of it."""
import ctypes

import numpy as np
import pytest

import loudness_helpers as lh
from conftest import synth

pytestmark = pytest.mark.gpu

R = 16
T_FULL = 33 * lh.B + 7
T_LIST = (0, 1, R, lh.CELL - 1, lh.CELL + 1, 4799, 4800, 4800 + R - 1, 4800 + R, 4800 + lh.CELL - 1, 4800 + lh.CELL + 1, 9601, T_FULL)
MONO = lh.PRESETS["mono"]


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import loudness
    return loudness


@pytest.fixture(scope="module")
def proto():
    from friture_amd.resample import Resampler
    return Resampler(48000, 192000, zeros=R).prototype


@pytest.fixture(scope="module")
def rec():
    """x32 [5, T] float32: noise, tone, chirp, an impulse at the last sample of sub-block 0, one at the first of sub-block 1.
    x64 [4, T] float64: noise, tone and chirp that are no float32 values, and DC 0.9 plus 1e-4 noise (the high-pass cancels
    a large state there).  y: the np.longdouble recurrence over all nine rows, float32 rows first."""
    rng = np.random.default_rng(5)
    x32 = np.zeros((5, T_FULL), np.float32)
    for s, kind in enumerate(("noise", "tone", "chirp")):
        x32[s] = synth(kind, T_FULL, 100 + s)
    x32[3, 4799] = 0.8
    x32[4, 4800] = -0.8
    x64 = np.empty((4, T_FULL))
    for s, kind in enumerate(("noise", "tone", "chirp")):
        x64[s] = synth(kind, T_FULL, 200 + s).astype(np.float64) * (1.0 + 1e-3 * rng.standard_normal(T_FULL))
    x64[3] = 0.9 + 1e-4 * rng.standard_normal(T_FULL)
    both = np.concatenate([x32.astype(np.float64), x64])
    return dict(x32=x32, x64=x64, both=both, y=lh.kweight(both, np.longdouble), tp={})


def reference(rec, proto, rows, T, weights=MONO, flush=True, tp_blocks=None):
    """lh.reference of the rows `rows` of the recording cut at T; the true peak only in the sub-blocks tp_blocks (default: all),
    nan elsewhere."""
    x = rec["both"][rows, :T]
    ref = lh.reference(x, weights, R, None, flush, y=rec["y"][rows, :T])
    npk = lh.emitted(T, R, flush)[1]
    tp = np.full((len(rows), npk), np.nan)
    for b in (range(npk) if tp_blocks is None else tp_blocks):
        key = (T, b)
        if key not in rec["tp"]:
            m0, m1 = 4 * lh.B * b, min(4 * lh.B * (b + 1), 4 * T)
            lo, hi = max(0, lh.B * b - 2 * R), min(T, lh.B * (b + 1) + 2 * R)
            # zeros beyond T and before 0 are the definition's; the window only spares gather the rest of the recording
            rec["tp"][key] = np.max(np.abs(lh.rh.gather(rec["both"][:, lo:hi], 4, 1, 4 * R, proto, m0, m1, k0=lo)), axis=1)
        tp[:, b] = rec["tp"][key][rows]
    ref["true_peak"] = tp
    return ref


def host(v):
    return v if isinstance(v, np.ndarray) or v is None else v.cpu().numpy()


def compare(res, ref, x, report=None):
    """Holds a result to the bars of the module docstring; returns the largest energy error as a share of its bar."""
    assert ref["margin"] > 1e-6, f"a block within {ref['margin']} LU of a threshold: choose another input"
    peak = np.max(np.abs(x.astype(np.float64)), axis=1, initial=0.0)
    energy, tp, sp = host(res.energy), host(res.true_peak), host(res.sample_peak)
    assert energy.shape == ref["energy"].shape and sp.shape == ref["sample_peak"].shape == tp.shape
    bar = 1e-10 * lh.B * peak ** 2
    err = np.abs(energy.astype(np.longdouble) - ref["energy"]).astype(np.float64)
    loud = peak > 0                                                  # a silent stream's bar is 0: it must come out exact
    assert np.all(err[~loud] == 0)
    share = float(np.max(err[loud] / bar[loud, None], initial=0.0))
    print(f"energy error / bar: {share:.3e}" + (f"  [{report}]" if report else ""))
    assert share <= 1.0
    assert np.array_equal(sp, ref["sample_peak"])
    known = ~np.isnan(ref["true_peak"])
    tp_err, tp_bar = np.abs(tp - ref["true_peak"])[known], 1e-12 * np.broadcast_to(peak[:, None], tp.shape)[known]
    print(f"true peak error / bar: {float(np.max(tp_err[tp_bar > 0] / tp_bar[tp_bar > 0], initial=0.0)):.3e}")
    assert np.all(tp_err <= tp_bar)
    for db, lin in ((host(res.true_peak_db), tp), (host(res.sample_peak_db), sp)):
        assert np.array_equal(db == -np.inf, lin == 0) and np.allclose(db[lin > 0], 20 * np.log10(lin[lin > 0]), rtol=0, atol=1e-9)
    for name in ("momentary", "short_term"):
        got, want = host(getattr(res, name)), ref[name]
        assert got.shape == want.shape, name
        above = want > -70.0
        assert np.array_equal(got > -70.0, above), name
        if above.any():
            print(f"{name} error: {float(np.max(np.abs(got[above] - want[above]))):.3e} LU")
            assert np.max(np.abs(got[above] - want[above])) <= 1e-6, name
    got, want = host(res.integrated), ref["integrated"]
    assert got.shape == want.shape and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-6) and np.all(got[~fin] == -np.inf)
    assert np.all(np.abs(host(res.loudness_range) - ref["loudness_range"]) <= 2e-6)
    return share


def pieces(batch, x, cuts, last_flush=True):
    """x cut at `cuts` (flush on the last piece): the per-call results concatenated along time, the last call's cumulative ones."""
    state, parts, res = None, [], None
    for a, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        res = batch.run(x[..., lo:hi], state, flush=last_flush and a == len(cuts) - 2)
        state = res.state
        parts.append(res)
    cat = {name: np.concatenate([host(getattr(p, name)) for p in parts], axis=-1) for name in ("momentary", "short_term", "energy", "true_peak", "sample_peak")}
    cat["integrated"], cat["loudness_range"] = host(res.integrated), host(res.loudness_range)
    return cat, state


def same_bits(cat, whole):
    for name, v in cat.items():
        w = host(getattr(whole, name))
        assert v.shape == w.shape and np.array_equal(v.view(np.uint64), w.view(np.uint64)), name


# ---- against the restatement --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", T_LIST)
def test_every_length_float32(mod, rec, proto, T):
    """Momentary and short-term come with 0, 1 and several entries; a partial last sub-block has peaks and no energy."""
    rows = [0, 1, 2, 3, 4]
    ref = reference(rec, proto, rows, T, tp_blocks=None if T < T_FULL else (0, 16, 32, 33))
    x = rec["x32"][:, :T]
    res = mod.LoudnessBatch("mono", tp_zeros=R).run(x)
    assert res.energy.shape == (5, T // lh.B) and res.true_peak.shape == (5, -(-T // lh.B))
    assert res.momentary.shape == (5, max(0, T // lh.B - 3)) and res.short_term.shape == (5, max(0, T // lh.B - 29))
    assert res.state.n_in == T and res.state.n_blocks == -(-T // lh.B)
    compare(res, ref, x, f"float32 T={T}")


@pytest.mark.parametrize("T", (4800 + R, 9601, T_FULL))
def test_float64_rows_and_the_dc_case(mod, rec, proto, T):
    """DC 0.9 + 1e-4 noise is where the cell form loses the most (measured on the CPU: 3.8e-13 absolute on the filtered
    samples); it must stay far inside the energy bar."""
    rows = [5, 6, 7, 8]
    ref = reference(rec, proto, rows, T, tp_blocks=None if T < T_FULL else (0, 1, 33))
    x = rec["x64"][:, :T]
    compare(mod.LoudnessBatch("mono", tp_zeros=R).run(x), ref, x, f"float64 T={T}")
    share = compare(mod.LoudnessBatch("mono", tp_zeros=R).run(x[3:]), {k: (v[3:] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}, x[3:], "DC alone")
    assert share < 0.1, "the DC case within 10x of the energy bar"


def test_cuda_tensors_give_the_bits_of_numpy_arrays(mod, rec, proto):
    import torch
    T = 9601
    for x in (rec["x32"][:, :T], rec["x64"][:, :T]):
        b = mod.LoudnessBatch("mono", tp_zeros=R)
        res_np, res_cu = b.run(x), b.run(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        assert all(isinstance(getattr(res_cu, n), torch.Tensor) and getattr(res_cu, n).is_cuda for n in res_cu._fields if n != "state")
        assert isinstance(res_cu.state.data, torch.Tensor) and isinstance(res_np.state.data, np.ndarray)
        # what the kernels write is the same to the bit; the dB values of the peaks and the loudness range are formed from it
        # with the log10 of the array's own library (torch on the device, numpy on the host), which may differ in the last place
        derived = ("true_peak_db", "sample_peak_db", "loudness_range")
        same_bits({n: host(getattr(res_cu, n)) for n in res_cu._fields if n != "state" and n not in derived}, res_np)
        for n in derived:
            assert np.allclose(host(getattr(res_cu, n)), getattr(res_np, n), rtol=0, atol=1e-12), n
        assert np.array_equal(host(res_cu.state.data), res_np.state.data)
    compare(res_cu, reference(rec, proto, [5, 6, 7, 8], T), x, "float64 CUDA tensor")
    # a state moves between the kinds
    first = b.run(x[:, :5000], flush=False)
    second = b.run(torch.from_numpy(np.ascontiguousarray(x[:, 5000:])).cuda(), first.state)
    assert np.array_equal(host(second.energy), res_np.energy[:, 1:]) and np.array_equal(host(second.integrated), res_np.integrated)


def test_impulses_on_either_side_of_a_sub_block_edge(mod, rec, proto):
    """An impulse at the last sample of sub-block 0 has its sample peak and its true peak there and only ringing in sub-block 1;
    one at the first sample of sub-block 1 the other way round."""
    T = 2 * lh.B + R
    res = mod.LoudnessBatch("mono", tp_zeros=R).run(rec["x32"][3:5, :T], flush=False)
    assert np.array_equal(res.sample_peak, [[np.float32(0.8), 0.0], [0.0, np.float32(0.8)]])
    top = float(np.float32(0.8)) * np.max(np.abs(proto))
    tp = res.true_peak
    assert abs(tp[0, 0] - top) <= 1e-15 and abs(tp[1, 1] - top) <= 1e-15 and 0 < tp[0, 1] < 0.5 * top and 0.5 * top < tp[1, 0] < top
    compare(res, reference(rec, proto, [3, 4], T, flush=False), rec["x32"][3:5, :T], "impulses")


def test_true_peak_is_the_resamplers_output(mod, rec):
    """Bit for bit: max |y| per 4 * 4800 outputs of Resampler(48000, 192000, zeros=tp_zeros).run, whole and cut."""
    from friture_amd.resample import Resampler
    T = 2 * lh.B + 333
    x = rec["x64"][:, :T]
    y = np.abs(Resampler(48000, 192000, zeros=R).run(x).y)
    want = np.stack([y[:, 4 * lh.B * b:4 * lh.B * (b + 1)].max(axis=1) for b in range(3)], axis=1)
    res = mod.LoudnessBatch("mono", tp_zeros=R).run(x)
    assert np.array_equal(res.true_peak, want)
    other = mod.LoudnessBatch("mono", tp_zeros=12).run(x)
    y = np.abs(Resampler(48000, 192000, zeros=12).run(x).y)
    assert np.array_equal(other.true_peak[:, 1], y[:, 4 * lh.B:8 * lh.B].max(axis=1)) and not np.array_equal(other.true_peak, res.true_peak)
    assert np.array_equal(other.energy, res.energy)


def test_relative_gate_over_ten_seconds(mod):
    """2 s at -36, 6 s at -23, 2 s at -36 LUFS, the right channel the left halved (exact in every precision): the gated value;
    the ungated mean lies 2 LU lower.  The reference filters the left row in np.longdouble, sample by sample."""
    amp = np.concatenate([np.full(96000, 10 ** -1.8), np.full(288000, 10 ** -1.15), np.full(96000, 10 ** -1.8)])
    left = (amp * lh.sine(1000.0, 480000)).astype(np.float32)
    x = np.stack([left, left * np.float32(0.5)])
    yl = lh.kweight_row(left, np.longdouble)
    y = np.stack([yl, yl * np.longdouble(0.5)])
    ref = lh.reference(x, lh.PRESETS["stereo"], R, None, y=y)
    ref["true_peak"] = np.full((2, 100), np.nan)
    res = mod.LoudnessBatch("stereo", tp_zeros=R).run(x)
    compare(res, ref, x, "10 s gate case")
    ungated = float(lh.lkfs(np.mean(ref["z400"][0].astype(np.float64))))
    assert 1.5 < res.integrated[0] - ungated < 2.5 and res.loudness_range[0] > 1.0
    assert mod.loudness(x, "stereo")[0] == res.integrated[0]


def test_silence(mod):
    res = mod.LoudnessBatch("stereo").run(np.zeros((2, 31 * lh.B), np.float32))
    assert np.all(res.momentary == -np.inf) and res.momentary.shape == (1, 28) and np.all(res.short_term == -np.inf) and res.short_term.shape == (1, 2)
    assert res.integrated[0] == -np.inf and res.loudness_range[0] == 0.0
    assert np.all(res.true_peak_db == -np.inf) and np.all(res.sample_peak_db == -np.inf) and np.all(res.energy == 0.0)


# ---- the same bits however the work is laid out ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def whole(mod, rec):
    return mod.LoudnessBatch("mono", tp_zeros=R).run(rec["x32"])


def test_random_partition_gives_the_bits_of_one_call(mod, rec, whole):
    rng = np.random.default_rng(9)
    cuts = [0] + sorted(rng.integers(0, T_FULL, 11).tolist()) + [T_FULL]
    cat, state = pieces(mod.LoudnessBatch("mono", tp_zeros=R), rec["x32"], cuts)
    same_bits(cat, whole)
    assert np.array_equal(state.data, whole.state.data) and state[1:] == whole.state[1:]


@pytest.mark.parametrize("t", T_LIST)
def test_a_cut_at_every_listed_length(mod, rec, whole, t):
    cat, _ = pieces(mod.LoudnessBatch("mono", tp_zeros=R), rec["x32"], [0, t, T_FULL])
    same_bits(cat, whole)


@pytest.mark.parametrize("size, T", [(1, lh.B + 2 * R + 3), (R - 1, 2 * lh.B + 100)])
def test_pieces_shorter_than_the_true_peak_reach(mod, rec, size, T):
    """Pieces of 1 sample across the end of a sub-block and its reach (a long first piece up to 10 samples before the edge),
    pieces of tp_zeros - 1 samples over two sub-blocks."""
    x = rec["x32"][:, :T]
    b = mod.LoudnessBatch("mono", tp_zeros=R)
    cuts = ([0] + list(range(lh.B - 10, T + 1))) if size == 1 else (list(range(0, T, size)) + [T])
    cat, _ = pieces(b, x, cuts)
    same_bits(cat, b.run(x))


def test_unflushed_pieces_hold_back_what_a_flush_releases(mod, rec, whole):
    b = mod.LoudnessBatch("mono", tp_zeros=R)
    first = b.run(rec["x32"][:, :lh.B + R - 1], flush=False)
    assert first.energy.shape == (5, 0) and first.state.n_blocks == 0
    second = b.run(rec["x32"][:, lh.B + R - 1:lh.B + R], first.state, flush=False)
    assert second.energy.shape == (5, 1) and np.array_equal(second.energy, whole.energy[:, :1]) and np.array_equal(second.true_peak, whole.true_peak[:, :1])
    with pytest.raises(ValueError, match="the state is final"):
        b.run(rec["x32"][:, :10], whole.state)
    with pytest.raises(ValueError, match="state of another shape"):
        b.run(rec["x32"][:2, :10], second.state)
    with pytest.raises(ValueError, match="state of another shape"):
        mod.LoudnessBatch("mono", tp_zeros=12).run(rec["x32"][:, :10], second.state)


def test_strided_views_single_rows_and_stream_counts(mod, rec):
    """A strided view is read in place; every row alone (S = 1) equals the same row inside S = 5."""
    T = 9601
    b = mod.LoudnessBatch("mono", tp_zeros=R)
    res = b.run(np.ascontiguousarray(rec["x32"][:, :T]))
    same_bits({n: host(getattr(b.run(rec["x32"][:, :T]), n)) for n in res._fields if n != "state"}, res)
    wide = np.zeros((10, T + 40), np.float32)
    wide[::2, 7:T + 7] = rec["x32"][:, :T]
    same_bits({n: host(getattr(b.run(wide[::2, 7:T + 7]), n)) for n in res._fields if n != "state"}, res)
    for s in range(5):
        one = b.run(rec["x32"][s, :T])
        for n in res._fields:
            if n != "state":
                assert np.array_equal(np.asarray(getattr(one, n)), getattr(res, n)[s]), (s, n)


def test_without_true_peak_the_energies_are_the_same(mod, rec):
    T = 4 * lh.B + 500
    with_tp = mod.LoudnessBatch("mono", tp_zeros=R).run(rec["x32"][:, :T])
    without = mod.LoudnessBatch("mono", tp_zeros=R, true_peak=False).run(rec["x32"][:, :T])
    assert without.true_peak is None and without.true_peak_db is None
    for n in ("energy", "sample_peak", "momentary", "integrated", "sample_peak_db"):
        assert np.array_equal(getattr(without, n), getattr(with_tp, n)), n


def test_programmes_of_5_1_ignore_the_lfe(mod, rec, proto):
    """[P, C, T] with "5.1": against the restatement's weighted sums, and the LFE row (weight 0) changes nothing."""
    import torch
    T = 7 * lh.B + R
    rows = [0, 1, 2, 5, 6, 7, 1, 0, 6, 2, 7, 5]
    x = rec["both"][rows, :T].reshape(2, 6, T)
    b = mod.LoudnessBatch("5.1", tp_zeros=R)
    res = b.run(x)
    assert res.momentary.shape == (2, 4) and res.integrated.shape == (2,) and res.energy.shape == (12, 7)
    compare(res, reference(rec, proto, rows, T, weights=lh.PRESETS["5.1"], tp_blocks=(0,)), x.reshape(12, T), "5.1")
    muted = x.copy()
    muted[:, 3] = 0.0
    other = b.run(muted)
    for n in ("momentary", "integrated", "loudness_range", "short_term"):
        assert np.array_equal(getattr(other, n), getattr(res, n)), n
    assert not np.array_equal(other.energy[3], res.energy[3])
    plain = mod.LoudnessBatch("5.0", tp_zeros=R).run(np.delete(x, 3, axis=1))
    assert np.array_equal(plain.momentary, res.momentary) and np.array_equal(plain.integrated, res.integrated)
    cu = b.run(torch.from_numpy(x).cuda()[:, :, 3:], flush=True)                   # a [P, C, T] view on the device
    assert np.array_equal(host(cu.energy), b.run(np.ascontiguousarray(x[:, :, 3:])).energy)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------

def test_c_abi_rejections(hip, proto):
    """Bad arguments: FRT_ERR_INVALID with a message that names the entry point, before any device call."""
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    w = np.ones(2)
    wp, pp = w.ctypes.data_as(dp), proto.ctypes.data_as(dp)

    def create(streams=4, channels=2, weights=wp, zeros=R, prototype=pp):
        h = vp()
        rc = hip.frt_loudness_create(ctypes.byref(h), streams, channels, weights, zeros, prototype)
        return rc, h, hip.frt_last_error().decode()

    for kwargs, word in ((dict(streams=0), "streams"), (dict(streams=3), "streams"), (dict(streams=65536), "streams"), (dict(channels=0), "channels"),
                         (dict(channels=65, streams=65), "channels"), (dict(zeros=0), "tp_zeros"), (dict(zeros=513), "tp_zeros"),
                         (dict(weights=None), "weights"), (dict(prototype=None), "prototype"),
                         (dict(weights=np.array([1.0, -1.0]).ctypes.data_as(dp)), "weight 1"),
                         (dict(weights=np.array([np.nan, 1.0]).ctypes.data_as(dp)), "weight 0"),
                         (dict(prototype=np.full(8 * R + 1, np.inf).ctypes.data_as(dp)), "prototype[0]")):
        rc, h, msg = create(**kwargs)
        assert rc == -1 and h.value is None and msg.startswith("frt_loudness_create") and word in msg, (kwargs, msg)
    assert hip.frt_loudness_create(None, 2, 2, wp, R, pp) == -1
    rc, h, _ = create()
    assert rc == 0 and h.value
    try:
        assert hip.frt_loudness_state_length(h, 0, 0) == 4 * (4 + R) and hip.frt_loudness_state_length(h, 33 * 4800 + 7, 32) == 4 * (4 + 4823 + 29) + 2 * 32
        assert hip.frt_loudness_state_length(h, 4799, 1) == -1 and hip.frt_loudness_state_length(None, 0, 0) == -1
        x, out, st, st2 = np.zeros((4, 100), np.float32), np.zeros(64), np.zeros(4 * (4 + R + 100)), np.zeros(4 * (4 + R + 100))
        ok = dict(x=x.ctypes.data, dtype=0, n=100, ld=100, state_in=None, state_out=st.ctypes.data, first_in=0, flush=0, true_peak=1, out=out.ctypes.data)
        for change, word in ((dict(dtype=2), "dtype"), (dict(n=-1), "bad input"), (dict(ld=99), "bad input"), (dict(x=None), "bad input"),
                             (dict(first_in=-1), "bad position"), (dict(first_in=100), "without its state"), (dict(flush=2), "flush"),
                             (dict(true_peak=-1), "true_peak"), (dict(state_out=None), "null"), (dict(out=None), "null"),
                             (dict(first_in=100, state_in=st.ctypes.data), "in place")):
            a = dict(ok, **change)
            rc = hip.frt_loudness_run(h, a["x"], a["dtype"], a["n"], a["ld"], a["state_in"], a["state_out"], a["first_in"], a["flush"], a["true_peak"], a["out"])
            msg = hip.frt_last_error().decode()
            assert rc == -1 and msg.startswith("frt_loudness_run") and word in msg, (change, msg)
        assert hip.frt_loudness_run(None, *[ok[k] for k in ("x", "dtype", "n", "ld", "state_in", "state_out", "first_in", "flush", "true_peak", "out")]) == -1
        assert hip.frt_loudness_set_stream(None, None) == -1
        a = ok
        assert hip.frt_loudness_run(h, a["x"], 0, 100, 100, None, st.ctypes.data, 0, 0, 1, out.ctypes.data) == 0
        assert hip.frt_loudness_run(h, a["x"], 0, 0, 100, st.ctypes.data, st2.ctypes.data, 100, 0, 1, out.ctypes.data) == 0
        assert np.array_equal(st, st2) and np.all(out[:2] == -np.inf) and np.all(st == 0.0)
    finally:
        hip.frt_loudness_destroy(h)
    hip.frt_loudness_destroy(None)
