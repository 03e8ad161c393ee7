"""Resampler on the GPU (resample.hip) against the numpy restatement of tests/resample_helpers.py, which test_resample_cpu.py
checks against a convolution, scipy's resample_poly and an analytic sine.  Seeded standard_normal input, S = 3 streams of
T = 5000 samples unless stated otherwise; every reference is computed once per (rate, T).

The float64 bar is the project's 1e-12 max|x|; the rounding bound of one output is K 2^-53 sum|c| = 513 * 1.1e-16 * 2.66 = 1.5e-13."""
import functools

import numpy as np
import pytest

import resample_helpers as H
from friture_amd import _batchio
from friture_amd.resample import Resampler, to_48k

pytestmark = pytest.mark.gpu

S, T = 3, 5000
PIECES = (0, 1, 60, 61, 2000, 2049, 5000)
# launch shapes the seven rates do not reach: at 352800 (L 20, M 147, K 941) the periods side by side in a workgroup are fewer than
# 256 threads' worth, because their span must fit LDS; at 3 840 000 (L 1, M 80, K 10241) not even one tile's span fits and the
# kernel reads the samples from memory instead
OTHER_SHAPES = ((352800, 5000), (3840000, 20011))


@functools.lru_cache(maxsize=None)
def design(rate):
    return Resampler(rate)


@functools.lru_cache(maxsize=None)
def samples(n=T, streams=S):
    x = np.random.default_rng(20240 + n).standard_normal((streams, n))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(rate, n=T, single=False):
    """The helper on samples(n) (single: rounded to float32 first, as a float32 recording holds them)."""
    r = design(rate)
    x = samples(n).astype(np.float32).astype(np.float64) if single else samples(n)
    y = np.stack([H.resample(row, r.L, r.M, r.C, r.prototype) for row in x])
    y.setflags(write=False)
    return y


def check64(y, rate, n=T, single=False):
    r, ref = design(rate), reference(rate, n, single)
    assert isinstance(y, np.ndarray) and y.dtype == np.float64 and y.shape == ref.shape == (S, -(-n * r.L // r.M))
    err, bar = np.max(np.abs(y - ref)), 1e-12 * np.max(np.abs(samples(n)))
    print(f"{rate}: max |y - helper| {err:.2e} (bar {bar:.2e})")
    assert err <= bar


# ---- parity -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", H.RATES)
def test_float64_parity(hip, rate):
    res = design(rate).run(samples())
    check64(res.y, rate)
    assert res.state.n_in == T and res.state.n_out == res.y.shape[1] and res.state.tail.shape == (S, design(rate).K - 1)


def test_float64_parity_cuda_tensor(hip):
    import torch
    x = torch.tensor(samples()).cuda()
    res = design(44100).run(x)
    assert res.y.is_cuda and res.y.dtype == torch.float64 and res.state.tail.is_cuda
    check64(res.y.cpu().numpy(), 44100)
    assert np.array_equal(x.cpu().numpy(), samples())


def test_output_count_that_is_no_whole_number_of_tiles_or_periods(hip):
    check64(design(44100).run(samples(20011)).y, 44100, 20011)


@pytest.mark.parametrize("rate,n", OTHER_SHAPES)
def test_float64_parity_other_launch_shapes(hip, rate, n):
    check64(design(rate).run(samples(n)).y, rate, n)


# ---- float32 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", (44100, 96000))
def test_float32_in_and_out(hip, rate):
    """One float32 rounding of the float64 sum, doubled because the float64 error may flip it."""
    y = design(rate).run(samples().astype(np.float32)).y
    ref = reference(rate, T, True).astype(np.float32)
    assert y.dtype == np.float32 and y.shape == ref.shape
    err, bar = np.max(np.abs(y.astype(np.float64) - ref.astype(np.float64))), 2.0 ** -23 * np.max(np.abs(y))
    print(f"{rate}: float32 max |y - float32(helper)| {err:.2e} (bar {bar:.2e})")
    assert err <= bar


def test_float32_in_float64_out(hip):
    check64(design(44100).run(samples().astype(np.float32), dtype=np.float64).y, 44100, T, True)
    import torch
    y = design(96000).run(torch.from_numpy(samples().astype(np.float32)).cuda(), dtype=torch.float64).y
    check64(y.cpu().numpy(), 96000, T, True)
    assert design(96000).run(samples(), dtype="float32").y.dtype == np.float32


# ---- pieces equal the whole, bit for bit ----------------------------------------------------------------------------------------------

def in_pieces(r, x, cuts, host_state_after=2):
    """x cut at `cuts`, flush on the last piece only; the state goes through to_host after piece `host_state_after`."""
    state, out = None, []
    for a, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        res = r.run(x[:, lo:hi], state=state, flush=a == len(cuts) - 2)
        state = _batchio.to_host(res.state) if a == host_state_after else res.state
        out.append(res.y)
    return out, state


@pytest.mark.parametrize("rate", (44100, 96000, 8000))
@pytest.mark.parametrize("kind", ("numpy", "cuda"))
def test_pieces_equal_the_whole_bit_for_bit(hip, rate, kind):
    r, x = design(rate), samples()
    if kind == "cuda":
        import torch
        x = torch.tensor(x).cuda()
    whole = _batchio.to_host(r.run(x).y)
    out, state = in_pieces(r, x, PIECES)
    out = [_batchio.to_host(o) for o in out]
    assert [o.shape for o in out[:3]] == [(S, 0)] * 3                       # shorter than the latency
    assert [o.shape[1] for o in out] == list(np.diff([r.n_out(c, c == T) for c in PIECES]))
    assert np.array_equal(np.concatenate(out, axis=1), whole)
    assert state.n_in == T and state.n_out == whole.shape[1]
    check64(whole, rate)


def test_a_row_does_not_depend_on_the_rows_beside_it(hip):
    for rate in (44100, 96000):
        r = design(rate)
        whole = r.run(samples()).y
        for s in range(S):
            assert np.array_equal(r.run(samples()[s:s + 1]).y, whole[s:s + 1])
            assert np.array_equal(r.run(samples()[s]).y, whole[s])              # the stream axis left out


def test_strided_cuda_view_is_read_in_place(hip):
    import torch
    big = torch.from_numpy(np.random.default_rng(5).standard_normal((S, 5200))).cuda()
    before = big.clone()
    view = big[:, 100:5100]
    assert not view.is_contiguous()
    r = design(44100)
    assert torch.equal(r.run(view).y, r.run(view.contiguous()).y)
    assert torch.equal(big, before)


# ---- edges --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", (44100, 96000, 8000))
def test_one_sample_and_a_flush_without_samples(hip, rate):
    r, x = design(rate), samples()
    one = r.run(x[:, :1])
    ref = np.stack([H.resample(row[:1], r.L, r.M, r.C, r.prototype) for row in x])
    assert one.y.shape == ref.shape == (S, -(-r.L // r.M))
    assert np.max(np.abs(one.y - ref)) <= 1e-12 * np.max(np.abs(x))
    first = r.run(x, flush=False)
    assert first.y.shape == (S, r.n_out(T, False)) and first.state.n_out == r.n_out(T, False)
    rest = r.run(x[:, :0], state=first.state, flush=True)
    assert rest.y.shape == (S, r.n_out(T) - r.n_out(T, False)) and rest.y.shape[1] > 0
    check64(np.concatenate([first.y, rest.y], axis=1), rate)
    with pytest.raises(ValueError, match="final"):
        r.run(x, state=rest.state)
    with pytest.raises(ValueError, match="another shape"):
        r.run(x[:2], state=first.state)


def test_to_48k(hip):
    x = samples()
    assert to_48k(x, 48000) is x
    assert np.array_equal(to_48k(x, 44100), design(44100).run(x).y)


# ---- quality on the device ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", (44100, 96000))
def test_a_sine_comes_out_as_the_analytic_sine(hip, rate):
    r = design(rate)
    err = H.sine_error(r.run(H.sine(rate)).y, r.L, r.M, r.C)
    print(f"{rate}: kernel - analytic sine {err:.2e}")
    assert err <= 2e-6
