"""TransferBatch on the GPU against the numpy restatement of its definition (tests/transfer_helpers.py), and against itself
for everything the definition says does not matter: cuts into calls, slab sizes, batch shapes, strides.

Bars (X1's): sxx, syy, sxy within 1e-12 of max_k Sxx, Syy, sqrt(Sxx Syy) of the estimate; h1 within 1e-10 max |h1|; coherence
within 1e-9.  The standard case asserts on its own reference the conditioning that makes the last two meaningful.  Every
parity test prints its distances before it asserts.  References are computed once per (N, hop, frames, streams) and shared."""
import functools

import numpy as np
import pytest

import transfer_helpers as th

pytestmark = pytest.mark.gpu

RUN = th.RUN


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import transfer
    return transfer


@functools.lru_cache(maxsize=None)
def case(N, hop, frames=40, streams=1):
    x = th.standard_case(N, hop, frames, streams)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case32(N, hop, frames=40, streams=1):
    x = case(N, hop, frames, streams).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(N, hop, frames, streams, average, f32):
    x = case32(N, hop, frames, streams) if f32 else case(N, hop, frames, streams)
    return th.restate_batch(x, N, hop, average=average)


def host(res):
    """The array fields of a TransferResult as numpy arrays."""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res._asdict().items() if k not in ("state", "freq")}


def on_device(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                 # a copy: the shared cases are read-only


def hold(res, ref, what):
    got = host(res)
    assert got["sxx"].shape == ref["sxx"].shape, (what, got["sxx"].shape, ref["sxx"].shape)
    assert got["frames"].tolist() == ref["frames"].tolist()
    d = th.distances(got, ref)
    print(what, " ".join(f"{k} {v:.2e}" for k, (v, _) in d.items()))
    for k, (v, bar) in d.items():
        assert v <= bar, (what, k, v, bar)
    return d


def same_bits(a, b, what=""):
    a, b = host(a), host(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def same_state(a, b):
    da, db = (s.data.cpu().numpy() if hasattr(s.data, "cpu") else s.data for s in (a, b))
    assert a[1:] == b[1:] and np.array_equal(da, db)


HOPS = {"N/4": lambda N: N // 4, "N/2": lambda N: N // 2, "3N/8+1": lambda N: 3 * N // 8 + 1, "N+N/8+3": lambda N: N + N // 8 + 3}


# ---- parity with the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop_rule", list(HOPS))
@pytest.mark.parametrize("N", [64, 512, 1024, 8192])
def test_parity_sizes_and_hops(mod, N, hop_rule):
    """Every size class (smallest wave-local, largest wave-local, first multi-wave, the LDS limit) at every hop class, the
    running estimate over 40 frames: float64 numpy rows alone, and three float32 streams on the device."""
    hop = HOPS[hop_rule](N)
    b = mod.TransferBatch(N, hop)
    hold(b.run(case(N, hop)), reference(N, hop, 40, 1, None, False), f"N {N} hop {hop} f64 numpy:")
    hold(b.run(on_device(case32(N, hop, 40, 3))), reference(N, hop, 40, 3, None, True), f"N {N} hop {hop} f32 cuda S 3:")


@pytest.mark.parametrize("average", [None, 1, RUN - 1, RUN, RUN + 1, 40])
@pytest.mark.parametrize("N", [64, 1024])
def test_parity_average(mod, N, average):
    hop = N // 2
    res = mod.TransferBatch(N, hop, average=average).run(on_device(case(N, hop, 40, 3)))
    ref = reference(N, hop, 40, 3, average, False)
    hold(res, ref, f"N {N} average {average}:")
    assert res.sxx.shape[1] == (1 if average is None else 40 // average)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_parity_dtypes_kinds_streams(mod, S, cuda, f32):
    N, hop = 512, 3 * 512 // 8 + 1
    x = (case32 if f32 else case)(N, hop, 40, S)
    res = mod.TransferBatch(N, hop, average=RUN + 1).run(on_device(x) if cuda else x)
    hold(res, reference(N, hop, 40, S, RUN + 1, f32), f"S {S} cuda {cuda} f32 {f32}:")
    import torch
    kind = torch.Tensor if cuda else np.ndarray
    assert all(isinstance(v, kind) for v in (res.sxx, res.syy, res.sxy, res.h1, res.coherence, res.frames, res.state.data))
    assert isinstance(res.freq, np.ndarray) and res.freq.shape == (N // 2 + 1,)
    assert "complex128" in str(res.sxy.dtype) and "complex128" in str(res.h1.dtype) and "float64" in str(res.coherence.dtype)


@pytest.mark.parametrize("frames", [RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, 2 * RUN + 1, 3 * RUN - 1, 3 * RUN, 3 * RUN + 1])
def test_parity_frame_counts_around_whole_runs(mod, frames):
    for N, hop in ((64, 32), (1024, 385)):
        x = case(N, hop, frames, 1)
        hold(mod.TransferBatch(N, hop).run(x), reference(N, hop, frames, 1, None, False), f"N {N} frames {frames} running:")
        hold(mod.TransferBatch(N, hop, average=frames).run(on_device(x)), reference(N, hop, frames, 1, frames, False),
             f"N {N} frames {frames} average {frames}:")


def test_explicit_window(mod):
    N, hop = 512, 256
    w = np.blackman(N) + 0.01
    x = case(N, hop)
    res = mod.TransferBatch(N, hop, window=w).run(x)
    hold(res, th.restate_batch(x, N, hop, window=w), "explicit window:")


def test_helpers(mod):
    N, hop = 64, 32
    for x in (case(N, hop), on_device(case(N, hop))):
        res = mod.TransferBatch(N, hop).run(x)
        h1 = host(res)["h1"]
        db, ph = mod.magnitude_db(res), mod.phase(res)
        assert type(db) is type(res.sxx) and type(ph) is type(res.sxx)
        db, ph = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (db, ph))
        assert np.allclose(db, 20 * np.log10(np.abs(h1)), rtol=0, atol=1e-12) and np.allclose(ph, np.angle(h1), rtol=0, atol=1e-12)


# ---- edge cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 512, 1024, 8192])
def test_dc_and_nyquist_bins(mod, N):
    """DC and a Nyquist-rate alternation of different amplitudes in the two rows (plus a little noise, so that every bin is
    defined): bins 0 and N/2, the two the two-for-one unpack treats apart, are checked on their own."""
    rng = np.random.default_rng(11)
    hop, T = N // 2, N + 19 * (N // 2)
    alt = 1.0 - 2.0 * (np.arange(T) % 2)
    x = np.stack([0.7 + 0.25 * alt + 1e-3 * rng.standard_normal(T), -0.3 + 0.5 * alt + 1e-3 * rng.standard_normal(T)])
    x = x.astype(np.float32).astype(np.float64)
    ref = th.restate_batch(x[None], N, hop)
    for inp in (x, on_device(x.astype(np.float32))):
        got = host(mod.TransferBatch(N, hop).run(inp))
        d = th.distances({k: v[None] for k, v in got.items()}, ref)
        print(f"N {N}:", " ".join(f"{k} {v:.2e}" for k, (v, _) in d.items()))
        for k in ("sxx", "syy", "sxy"):
            assert d[k][0] <= d[k][1], (k, d[k])
        for k in (0, N // 2):
            r = {name: ref[name][0, 0, k] for name in ("sxx", "syy", "sxy", "h1", "coherence")}
            assert abs(got["sxx"][0, k] - r["sxx"]) <= 1e-12 * r["sxx"] and abs(got["syy"][0, k] - r["syy"]) <= 1e-12 * r["syy"]
            assert abs(got["sxy"][0, k] - r["sxy"]) <= 1e-12 * abs(r["sxy"])
            assert abs(got["h1"][0, k] - r["h1"]) <= 1e-10 * abs(r["h1"]) and abs(got["coherence"][0, k] - r["coherence"]) <= 1e-9
            assert abs(got["h1"][0, k].imag) <= 1e-10 * abs(r["h1"])
        assert abs(got["h1"][0, 0].real - (-0.3 / 0.7)) < 5e-3 and abs(got["h1"][0, N // 2].real - 2.0) < 2e-2


@pytest.mark.parametrize("d", [37, -37])
@pytest.mark.parametrize("N", [64, 1024])
def test_delay_aligns_a_shifted_copy(mod, N, d):
    """y[t] = x[t - d] measured with delay = d is the identity system; with delay = 0 it is not, which pins the sign."""
    rng = np.random.default_rng(12)
    hop, T = N // 2, N + 20 * (N // 2) + 37
    x = rng.standard_normal(T)
    y = np.concatenate([np.zeros(37), x[:-37]]) if d > 0 else np.concatenate([x[37:], np.zeros(37)])
    pair = np.stack([x, y])[None]
    ref = th.restate_batch(pair, N, hop, delay=d)
    for inp in (pair, on_device(pair)):
        res = mod.TransferBatch(N, hop, delay=d).run(inp)
        hold(res, ref, f"N {N} delay {d}:")
        got = host(res)
        assert got["frames"].tolist() == [21]
        assert np.max(np.abs(got["h1"] - 1)) <= 1e-10 and np.max(np.abs(got["coherence"] - 1)) <= 1e-9
    off = host(mod.TransferBatch(N, hop, delay=0).run(pair))
    assert np.max(np.abs(off["h1"] - 1)) > 0.1


@pytest.mark.parametrize("N", [64, 1024])
def test_a_silent_row_gives_zeros_not_nan(mod, N):
    rng = np.random.default_rng(13)
    T = N + 20 * (N // 2)
    x = rng.standard_normal(T)
    for pair in (np.stack([x, np.zeros(T)]), np.stack([np.zeros(T), x]), np.zeros((2, T))):
        for average in (None, 4):
            got = host(mod.TransferBatch(N, average=average).run(on_device(pair)))
            assert np.all(got["h1"] == 0) and np.all(got["coherence"] == 0)
            assert all(np.all(np.isfinite(got[k])) for k in ("sxx", "syy", "sxy", "h1", "coherence"))
            assert np.all(got["sxx"] > 0) == bool(pair[0].any()) and np.all(got["syy"] > 0) == bool(pair[1].any())


@pytest.mark.parametrize("N", [64, 512, 1024, 8192])
def test_a_single_frame_is_coherent(mod, N):
    x = case(N, N // 2)[0, :, :N + N // 2 - 1]
    got = host(mod.TransferBatch(N).run(x))
    assert got["frames"].tolist() == [1] and np.max(np.abs(got["coherence"] - 1)) <= 1e-9


def test_too_few_samples_give_no_estimate_and_a_state_that_continues(mod):
    N, hop = 512, 256
    x = on_device(case(N, hop, 40, 3))
    for average in (None, 2):
        b = mod.TransferBatch(N, hop, average=average, delay=5)
        first = b.run(x[:, :, :N + 4])
        assert first.sxx.shape == (3, 0, N // 2 + 1) and first.h1.shape == (3, 0, N // 2 + 1) and first.frames.shape == (0,)
        assert first.state.n_in == N + 4 and first.state.pending == N + 4
        empty = b.run(x[:, :, :0], first.state)
        assert empty.sxx.shape[1] == 0
        same_state(empty.state, first.state)
        whole = b.run(x)
        rest = b.run(x[:, :, N + 4:], first.state)
        same_bits(rest, whole)
        same_state(rest.state, whole.state)


# ---- bit identity, GPU against GPU ----------------------------------------------------------------------------------------------

def in_pieces(b, x, cuts, **kw):
    """The results of x [.., T] fed in the pieces between `cuts`, and the last state."""
    state, out, edges = None, [], [0, *cuts, x.shape[-1]]
    for lo, hi in zip(edges[:-1], edges[1:]):
        res = b.run(x[..., lo:hi], state, **kw)
        state = res.state
        out.append(res)
    return out


def joined(results):
    cat = (lambda v: np.concatenate(v, axis=-2))
    return {k: cat([host(r)[k] for r in results]) for k in ("sxx", "syy", "sxy", "h1", "coherence")}


@pytest.mark.parametrize("average", [None, 5, RUN + 1])
@pytest.mark.parametrize("N, hop", [(64, 24), (1024, 512), (512, 700)])
def test_pieces_cut_anywhere_give_the_bits_of_one_call(mod, N, hop, average):
    x = on_device(case32(N, hop, 40, 2))
    T = x.shape[-1]
    b = mod.TransferBatch(N, hop, average=average, delay=-3)
    whole = b.run(x)
    edge = N + 3 + 9 * hop                                       # frame 9 completes with sample edge - 1
    for cuts in ((1,), (T - 1,), (edge - 1,), (edge,), (edge + 1,), (N + 3 + 21 * hop + 7,), (1, 2, edge - 1, edge, edge + 1, T - 1)):
        parts = in_pieces(b, x, cuts)
        same_state(parts[-1].state, whole.state)
        if average is None:
            same_bits(parts[-1], whole, cuts)
        else:
            got, want = joined(parts), host(whole)
            for k in got:
                assert np.array_equal(got[k], want[k]), (cuts, k)
            assert sum(int(p.frames.shape[0]) for p in parts) == whole.frames.shape[0]


def test_one_sample_pieces(mod):
    N, hop = 64, 16
    x = case(N, hop, RUN + 3, 1)
    for average in (None, 3):
        b = mod.TransferBatch(N, hop, average=average)
        whole = b.run(x)
        parts = in_pieces(b, x, range(1, x.shape[-1]))
        same_state(parts[-1].state, whole.state)
        if average is None:
            same_bits(parts[-1], whole)
        else:
            assert np.array_equal(joined(parts)["sxy"], host(whole)["sxy"]) and np.array_equal(joined(parts)["coherence"], host(whole)["coherence"])


@pytest.mark.parametrize("average", [None, 1, RUN + 1])
@pytest.mark.parametrize("N", [64, 1024])
def test_slab_size_does_not_matter(mod, N, average):
    hop = N // 4
    x = on_device(case(N, hop, 40, 3))
    b = mod.TransferBatch(N, hop, average=average)
    whole = b.run(x)
    run_bytes = 3 * (N // 2 + 1) * 4 * 8
    for scratch in (0, run_bytes, 2 * run_bytes + 1):            # one run per slab (3 or more slabs), one, two
        res = b.run(x, scratch_bytes=scratch)
        same_bits(res, whole, scratch)
        same_state(res.state, whole.state)
    parts = in_pieces(b, x, (N + 17 * hop + 5,), scratch_bytes=run_bytes)
    same_state(parts[-1].state, whole.state)


def test_shapes_strides_and_batches(mod):
    import torch
    N, hop = 512, 193
    x = case(N, hop, 40, 3)
    T = x.shape[-1]
    b = mod.TransferBatch(N, hop, average=7)
    whole = b.run(on_device(x))
    # [2, T] against [1, 2, T]; stream s of the batch against the same stream alone
    for s in range(3):
        alone, flat = b.run(on_device(x[s:s + 1])), b.run(on_device(x[s]))
        assert flat.sxx.shape == (5, N // 2 + 1) and alone.sxx.shape == (1, 5, N // 2 + 1)
        for k in ("sxx", "syy", "sxy", "h1", "coherence"):
            assert torch.equal(getattr(alone, k)[0], getattr(flat, k)) and torch.equal(getattr(alone, k)[0], getattr(whole, k)[s]), (s, k)
    # strided views against contiguous copies: device and host
    wide = np.zeros((3, 3, T + 5))
    wide[:, ::2, 3:3 + T] = x
    for base in (wide, on_device(wide)):
        view = base[:, ::2, 3:3 + T]
        assert not (view.flags.c_contiguous if isinstance(view, np.ndarray) else view.is_contiguous())
        same_bits(b.run(view), whole, "view")
    swapped = on_device(np.ascontiguousarray(x.transpose(1, 0, 2))).permute(1, 0, 2)      # pair stride < row stride
    same_bits(b.run(swapped), whole, "permuted")
    same_bits(b.run(x), whole, "numpy")


def test_a_side_stream_is_ordered_behind_the_callers_work(mod):
    import torch
    N, hop = 1024, 512
    x = on_device(case(N, hop))
    want = mod.TransferBatch(N, hop).run(x)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y = x * 2.0
        got = mod.TransferBatch(N, hop).run(y)
        ratio = got.sxx / want.sxx
    side.synchronize()
    assert torch.allclose(ratio, torch.full_like(ratio, 4.0), rtol=1e-12, atol=0)
