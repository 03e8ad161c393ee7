"""ConvolveBatch on the GPU against the numpy restatement of its definition (tests/convolve_helpers.py), and against itself
for everything the definition says does not matter: cuts into calls, slab sizes, tiles, batch shapes, strides.

The bar (X2's): every row within 1e-12 max|x| sum|h| of the direct sum in np.longdouble.  Every parity test prints its distance
before it asserts.  Inputs and references are made once per shape and shared, read-only."""
import functools

import numpy as np
import pytest

import convolve_helpers as ch

pytestmark = pytest.mark.gpu

J = 2                                       # the block kernel's tile (convolve.TILE)


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import convolve
    assert convolve.TILE == J
    return convolve


@functools.lru_cache(maxsize=None)
def case(S, T, L, per_stream=False, f32=False):
    """(x [S, T], h [L] or [S, L], the longdouble reference [S, T + L - 1])."""
    x = ch.signal(T + 7 * L, S, T, np.float32 if f32 else np.float64)
    h = ch.taps(L, L, S if per_stream else None)
    ref = ch.restate_long(x, h)
    ref.setflags(write=False)
    return x, h, ref


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def on_device(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                 # a copy: the shared cases are read-only


def hold(y, x, h, ref, what):
    d = ch.distance(host(y), x, h, ref)
    print(f"{what} {d:.2e}")
    assert d <= ch.BAR, (what, d)
    return d


def in_pieces(b, x, cuts, last_flush=True, **kw):
    """The outputs of x [.., T] fed in the pieces between `cuts` (all but the last without a flush), joined, and the results."""
    state, out, edges = None, [], [0, *cuts, x.shape[-1]]
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        res = b.run(x[..., lo:hi], state, flush=last_flush and k == len(edges) - 2, **kw)
        state = res.state
        out.append(res)
    return np.concatenate([host(r.y) for r in out], axis=-1), out


# ---- parity with the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 63, 64, 65, 129, 200])
def test_parity_partition_counts_and_lengths(mod, L):
    """B = 64: P = 1, 1, 1, 2, 3, 4 at recordings shorter than, equal to and longer than a block."""
    b = mod.ConvolveBatch(case(1, 64, L)[1], block=64)
    assert b.partitions == -(-L // 64)
    for T in (1, 63, 64, 65, 129, 1000):
        x, h, ref = case(1, T, L)
        assert np.array_equal(h, b.taps[0])
        hold(b.run(x).y, x, h, ref, f"B 64 L {L} T {T}:")


def test_parity_many_partitions(mod):
    x, h, ref = case(1, 5000, 2560)
    b = mod.ConvolveBatch(h, block=64)
    assert b.partitions == 40
    hold(b.run(on_device(x)).y, x, h, ref, "B 64 L 2560 T 5000:")


@pytest.mark.parametrize("B", [128, 256, 512, 1024, 2048, 4096])
def test_parity_every_block_size(mod, B):
    x, h, ref = case(2, 3 * B + 5, B + 1, per_stream=True)
    b = mod.ConvolveBatch(h, block=B)
    assert b.partitions == 2
    hold(b.run(on_device(x)).y, x, h, ref, f"B {B} L {B + 1} T {3 * B + 5} S 2:")


@pytest.mark.parametrize("blocks", [J - 1, J, J + 1, 2 * J + 1])
def test_parity_tile_edges(mod, blocks):
    """A launch of J - 1, J, J + 1 and 2 J + 1 output blocks: flushed (the last block is short) and not (all are whole)."""
    B, L = 64, 10
    x, h, ref = case(1, blocks * B - L, L)
    assert -(-(x.shape[1] + L - 1) // B) == blocks
    hold(mod.ConvolveBatch(h, block=B).run(x).y, x, h, ref, f"{blocks} blocks, flushed:")
    L = 70
    x, h, ref = case(1, blocks * B, L)
    res = mod.ConvolveBatch(h, block=B).run(x, flush=False)
    assert res.y.shape == (1, blocks * B) and res.state.n_out == blocks * B
    hold(res.y, x, h, ref[:, :blocks * B], f"{blocks} blocks, not flushed:")


# ---- kinds ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("per_stream", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_parity_dtypes_kinds_streams_filters(mod, S, per_stream, cuda, f32):
    import torch
    x, h, ref = case(S, 700, 150, per_stream, f32)
    b = mod.ConvolveBatch(h, block=64)
    res = b.run(on_device(x) if cuda else x)
    assert isinstance(res.y, torch.Tensor if cuda else np.ndarray) and res.state.tail is None
    assert tuple(res.y.shape) == (S, 849) and str(res.y.dtype).split(".")[-1] == ("float32" if f32 else "float64")
    if f32:                                  # one rounding of the float64 value of the same call
        wide = b.run(on_device(x) if cuda else x, dtype=np.float64 if not cuda else torch.float64)
        assert str(wide.y.dtype).split(".")[-1] == "float64"
        hold(wide.y, x, h, ref, f"S {S} per-stream {per_stream} cuda {cuda} f32 in, f64 out:")
        assert np.array_equal(host(res.y), host(wide.y).astype(np.float32))
    else:
        hold(res.y, x, h, ref, f"S {S} per-stream {per_stream} cuda {cuda} f64:")
        narrow = b.run(on_device(x) if cuda else x, dtype="float32")
        assert np.array_equal(host(narrow.y), host(res.y).astype(np.float32))


def test_shapes_strides_and_batches(mod):
    import torch
    x, h, ref = case(3, 700, 150, True)
    b = mod.ConvolveBatch(h, block=64)
    whole = host(b.run(on_device(x)).y)
    hold(whole, x, h, ref, "S 3:")
    for s in range(3):                       # a stream alone, as [1, T] and as [T], against the batch
        alone = mod.ConvolveBatch(h[s], block=64)
        flat, one = alone.run(on_device(x[s])), alone.run(x[s:s + 1])
        assert tuple(flat.y.shape) == (849,) and one.y.shape == (1, 849)
        assert np.array_equal(host(flat.y), whole[s]) and np.array_equal(one.y[0], whole[s])
        assert np.array_equal(host(mod.convolve(on_device(x[s]), h[s], block=64)), whole[s])
    wide = np.zeros((3, 2, 710))
    wide[:, 0, 3:703] = x
    for base in (wide, on_device(wide)):     # strided views against contiguous copies: host and device
        view = base[:, 0, 3:703]
        assert not (view.flags.c_contiguous if isinstance(view, np.ndarray) else view.is_contiguous())
        assert np.array_equal(host(b.run(view).y), whole)
    same = mod.ConvolveBatch(h[1], block=64)
    want = host(same.run(x[1]).y)
    for view in (np.broadcast_to(x[1], (3, 700)), on_device(x[1]).expand(3, 700)):      # overlapping rows are made contiguous
        got = host(same.run(view).y)
        assert got.shape == (3, 849) and all(np.array_equal(got[s], want) for s in range(3))
    assert isinstance(mod.convolve(x[0], h[0]), np.ndarray) and isinstance(mod.convolve(on_device(x[0]), h[0]), torch.Tensor)


# ---- bit identity, GPU against GPU ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuda", [False, True])
def test_pieces_cut_anywhere_give_the_bits_of_one_call(mod, cuda):
    B, L, T = 64, 70, 1000
    x, h, ref = case(2, T, L, True, True)
    xin = on_device(x) if cuda else x
    b = mod.ConvolveBatch(h, block=B)
    whole = host(b.run(xin).y)
    rng = np.random.default_rng(5)
    fixed = [(1,), (T - 1,), (B - 1,), (B,), (B + 1,), (3 * B, 3 * B), (1, 2, B - 1, B, B + 1, 2 * B + 1, 9 * B, T - 1)]
    drawn = [tuple(sorted(rng.integers(0, T + 1, size=k).tolist())) for k in (1, 2, 3, 7, 20, 20)]
    for cuts in fixed + drawn:
        got, parts = in_pieces(b, xin, cuts)
        assert got.shape == whole.shape and np.array_equal(got, whole), cuts
        n = 0
        for r in parts[:-1]:                 # the counts and the state of every call on the way
            n = r.state.n_in
            assert r.state.n_out == (n // B) * B and np.array_equal(host(r.state.tail), ch.state_after(x[:, :n], L, B)), (cuts, n)
        assert parts[-1].state.tail is None and parts[-1].state.n_out == T + L - 1


def test_one_sample_pieces(mod):
    B, L, T = 64, 70, 200
    x, h, ref = case(1, T, L)
    b = mod.ConvolveBatch(h, block=B)
    whole = b.run(x).y
    got, _ = in_pieces(b, x, range(1, T))
    assert np.array_equal(got, whole)


def test_unflushed_pieces_and_an_empty_flushed_call(mod):
    B, L, T = 64, 70, 1000
    x, h, ref = case(2, T, L, True, True)
    xin = on_device(x)
    b = mod.ConvolveBatch(h, block=B)
    whole = host(b.run(xin).y)
    got, parts = in_pieces(b, xin, (333, 334, 700), last_flush=False)
    assert got.shape == (2, (T // B) * B) and np.array_equal(got, whole[:, :got.shape[1]])
    last = b.run(xin[:, :0], parts[-1].state, flush=True)
    assert np.array_equal(np.concatenate([got, host(last.y)], axis=-1), whole)
    with pytest.raises(ValueError, match="flushed"):
        b.run(xin[:, :0], last.state)


@pytest.mark.parametrize("B, L", [(64, 200), (1024, 1025)])
def test_slab_size_does_not_matter(mod, B, L):
    x, h, ref = case(2, 3 * 1024 + 5, L, True)
    xin = on_device(x)
    b = mod.ConvolveBatch(h, block=B)
    whole = host(b.run(xin).y)
    win = 2 * (B + 1) * 16                                       # one window of both streams
    for scratch in (0, b.partitions * win, (b.partitions + 2) * win + 1):     # one block per launch, one, three
        assert np.array_equal(host(b.run(xin, scratch_bytes=scratch).y), whole), scratch
    got, _ = in_pieces(b, xin, (B + 17, 2 * B + 1), scratch_bytes=0)
    assert np.array_equal(got, whole)


# ---- exactness ------------------------------------------------------------------------------------------------------------------

def test_a_silent_row_gives_exact_zeros(mod):
    x, h, ref = case(3, 700, 150)
    x = np.array(x)
    x[1] = 0.0
    for B in (64, 256):
        y = host(mod.ConvolveBatch(h, block=B).run(on_device(x)).y)
        assert not y[1].any() and y[0].any() and y[2].any()
    assert not host(mod.convolve(np.zeros(5000, np.float32), ch.taps(9, 5000))).any()


def test_less_than_a_block_gives_no_output_and_a_state_that_continues(mod):
    B, L = 128, 300
    x, h, ref = case(2, 1000, L)
    xin = on_device(x)
    b = mod.ConvolveBatch(h, block=B)
    first = b.run(xin[:, :B - 1], flush=False)
    assert tuple(first.y.shape) == (2, 0) and first.state.n_in == B - 1 and first.state.n_out == 0
    assert np.array_equal(host(first.state.tail), x[:, :B - 1])
    empty = b.run(xin[:, :0], first.state, flush=False)
    assert tuple(empty.y.shape) == (2, 0) and np.array_equal(host(empty.state.tail), x[:, :B - 1]) and empty.state[1:] == first.state[1:]
    rest = b.run(xin[:, B - 1:], first.state)
    assert np.array_equal(host(rest.y), host(b.run(xin).y))
    flat = b.run(x[0, :5], flush=False)
    assert flat.y.shape == (0,) and flat.y.dtype == np.float64 and flat.state.tail.shape == (1, 5)


# ---- the impulse response and the round trip ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 1024, 8192])
def test_impulse_response_equals_numpys_irfft(mod, N):
    """A sample of irfft(H) is bounded by (2 / N) sum|H|; a float64 transform of 13 levels rounds some 1e-15 of that, so the
    package's float64 bar of 1e-12 of that scale holds both transforms with room."""
    rng = np.random.default_rng(N)
    H = rng.standard_normal((2, 3, N // 2 + 1)) + 1j * rng.standard_normal((2, 3, N // 2 + 1))
    want = np.fft.irfft(H, N)
    bar = 1e-12 * 2.0 * np.mean(np.abs(H), axis=-1, keepdims=True)
    for inp in (H, on_device(H), H[0, 0], on_device(H)[1]):
        got = mod.impulse_response(inp)
        assert type(got) is type(inp) and "float64" in str(got.dtype)
        ref = want if got.ndim == 3 else (want[0, 0] if got.ndim == 1 else want[1])
        lim = bar if got.ndim == 3 else (bar[0, 0] if got.ndim == 1 else bar[1])
        d = np.abs(host(got) - ref)
        print(f"N {N} {tuple(got.shape)}: {np.max(d / lim) * 1e-12:.2e} of the scale")
        assert got.shape == ref.shape and np.all(d <= lim)
    assert mod.impulse_response(H[:0]).shape == (0, 3, N)


def test_round_trip_measure_invert_apply(mod):
    """TransferBatch measures a known 32-tap FIR on 2^16 samples of white noise (fft_size 1024), impulse_response recovers the
    taps, ConvolveBatch with them reproduces the measured row.  The estimate's own error dominates: the same three steps in
    numpy miss the taps by 3.9e-4 and the row by 4.0e-3 (max|y| = 12.1); the device may miss by ten times that."""
    import transfer_helpers as th
    from friture_amd import transfer
    rng = np.random.default_rng(77)
    T, N = 1 << 16, 1024
    fir = rng.standard_normal(32) * np.exp(-np.arange(32) / 8.0)
    x = rng.standard_normal(T)
    y = np.convolve(x, fir)[:T]
    ir_np = np.fft.irfft(th.restate(x, y, N, N // 2)["h1"][0], N)
    taps_np, row_np = np.max(np.abs(ir_np[:32] - fir)), np.max(np.abs(np.convolve(x, ir_np[:32])[:T] - y))
    pair = on_device(np.stack([x, y]))
    ir = mod.impulse_response(transfer.TransferBatch(N, N // 2).run(pair))
    assert tuple(ir.shape) == (1, N)
    taps = host(ir)[0, :32]
    got = mod.ConvolveBatch(taps).run(pair[0], flush=False)
    assert tuple(got.y.shape) == (T,)
    taps_gpu, row_gpu = np.max(np.abs(taps - fir)), np.max(np.abs(host(got.y) - y))
    print(f"taps: numpy {taps_np:.2e}, device {taps_gpu:.2e}; row: numpy {row_np:.2e}, device {row_gpu:.2e}")
    assert taps_gpu <= 10 * taps_np and row_gpu <= 10 * row_np
    # X1 holds h1 within 1e-10 max|h1| per bin, and a sample of irfft(E) is at most (2 / N) sum|E|
    assert np.max(np.abs(host(ir)[0] - ir_np)) <= 2e-10 * np.max(np.abs(np.fft.rfft(ir_np)))


# ---- stream order ---------------------------------------------------------------------------------------------------------------

def test_a_side_stream_is_ordered_behind_the_callers_work(mod):
    import torch
    x, h, ref = case(2, 3 * 1024 + 5, 1025, True)
    xin = on_device(x)
    b = mod.ConvolveBatch(h)
    want = b.run(xin).y
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        doubled = xin * 2.0
        got = b.run(doubled).y
        same = torch.equal(got, want * 2.0)
    side.synchronize()
    assert bool(same)
