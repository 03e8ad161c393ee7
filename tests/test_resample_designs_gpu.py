"""Resampler on the GPU away from the default designs: short and asymmetric prototypes through the C entry points
(resample_helpers.Device), every launch class of resample_helpers.ROWS (test_resample_cpu.py holds each row to the class it is
there for), stream positions up to the 2^40 the entry point admits, padded layouts and the largest stream count.

Every comparison is against resample_helpers.reference_and_bound: the definition of include/friture_hip.h summed in extended
precision, and the a-priori rounding bound B of the one fma chain per output that the kernel promises.  Nothing here is a
measured tolerance: |y - ref| <= B for float64, B + 2^-24 (|ref| + B) for a float32 output.  Seeded standard_normal samples
and, through Device, seeded standard_normal prototypes: h[i] != h[2C - i], O(1) at both ends."""
import functools
from pathlib import Path

import numpy as np
import pytest

import resample_helpers as H
from friture_amd import _lib
from friture_amd.resample import Resampler, ResampleState

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
S = 2
DESIGNS = tuple(row[0] for row in H.ROWS)
# the rows the public class can express, with its own Kaiser prototype: (arguments, zeros) -> (L, M, C)
CLASS_ROWS = (((32000,), 1, (3, 2, 3)), ((44100,), 4, (160, 147, 640)), ((48000, 44100), 2, (147, 160, 320)),
              ((3, 1000), 4, (1000, 3, 4000)), ((1499, 601), 4, (601, 1499, 5996)), ((22051,), 8, (48000, 22051, 384000)),
              ((72000,), 5, (2, 3, 15)), ((144000,), 64, (1, 3, 192)))
SENTINEL = -12345.678


def name(design):
    return "-".join(map(str, design))


@functools.lru_cache(maxsize=None)
def constants():
    return H.kernel_constants((ROOT / "friture_amd" / "csrc" / "resample.hip").read_text())


@functools.lru_cache(maxsize=None)
def plan(L, M, C):
    return H.launch_plan(L, M, C, *constants())


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def prototype(C):
    return frozen(np.random.default_rng(7000 + C).standard_normal(2 * C + 1))


@functools.lru_cache(maxsize=None)
def device(L, M, C, streams=S):
    return H.Device(L, M, C, prototype(C), streams)


@functools.lru_cache(maxsize=None)
def samples(L, M, C, streams=S):
    n = H.row_length(L, M, plan(L, M, C)["np"], constants()[0])
    return frozen(np.random.default_rng(L + M + C).standard_normal((streams, n)))


def rounded(x):
    """x as a float32 recording holds it."""
    return x.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(L, M, C, single=False, streams=S):
    """(ref, B) of the whole flushed stream samples(L, M, C) under prototype(C)."""
    x = samples(L, M, C, streams)
    return H.reference_and_bound(rounded(x) if single else x, L, M, C, prototype(C), 0, H.count(x.shape[1], L, M, C, True))


def within(y, ref, B, what):
    worst = H.excess(y, ref, B)
    print(f"{what}: max |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, what


def tails_are_the_last_inputs(x, cuts, states, K):
    """After every piece: the last K - 1 inputs so far, zeros before the stream's start, exactly."""
    padded = np.concatenate([np.zeros((x.shape[0], K - 1)), x], axis=1)
    for hi, (tail, n_in, _) in zip(cuts[1:], states):
        assert n_in == hi and np.array_equal(tail, padded[:, hi:hi + K - 1]), hi


# ---- the design table, asymmetric prototypes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("design", DESIGNS, ids=name)
def test_design_row_whole_and_in_pieces(hip, design):
    d, x, K = device(*design), samples(*design), plan(*design)["K"]
    whole, state = d.run(x)
    ref, B = reference(*design)
    assert whole.shape == ref.shape and state[1:] == (x.shape[1], whole.shape[1])
    within(whole, ref, B, f"L, M, C = {design}, K = {K}, float64")
    cuts = H.piece_cuts(x.shape[1], K)
    out, states = d.pieces(x, cuts)
    assert [o.shape[1] for o in out] == list(np.diff([d.n_out(c, a == len(cuts) - 1) for a, c in enumerate(cuts)]))
    assert np.array_equal(np.concatenate(out, axis=1), whole)
    tails_are_the_last_inputs(x, cuts, states, K)


@pytest.mark.parametrize("out", (np.float32, np.float64), ids=("float32-out", "float64-out"))
@pytest.mark.parametrize("design", ((3, 2, 12), (601, 1499, 5996)), ids=name)
def test_design_row_float32_in(hip, design, out):
    d, x = device(*design), samples(*design).astype(np.float32)
    whole, _ = d.run(x, out=out)
    ref, B = reference(*design, single=True)
    assert whole.dtype == out and whole.shape == ref.shape
    within(whole, ref, B, f"L, M, C = {design}, float32 in, {np.dtype(out).name} out")
    cuts = H.piece_cuts(x.shape[1], d.K)
    pieces, states = d.pieces(x, cuts, out=out)
    assert np.array_equal(np.concatenate(pieces, axis=1), whole)
    tails_are_the_last_inputs(x.astype(np.float64), cuts, states, d.K)


# ---- the same classes through the public class, with its Kaiser prototype ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def resampler(args, zeros):
    return Resampler(*args, zeros=zeros)


@pytest.mark.parametrize("args,zeros,design", CLASS_ROWS, ids=[name(row[2]) for row in CLASS_ROWS])
def test_resampler_passes_rate_out_and_zeros_through(hip, args, zeros, design):
    r = resampler(args, zeros)
    assert (r.L, r.M, r.C) == design and r.K == plan(*design)["K"]
    x = samples(*design)
    whole = r.run(x)
    ref, B = H.reference_and_bound(x, r.L, r.M, r.C, r.prototype, 0, r.n_out(x.shape[1]))
    assert whole.y.shape == ref.shape and whole.state.n_in == x.shape[1] and whole.state.n_out == ref.shape[1]
    within(whole.y, ref, B, f"Resampler{args}, zeros {zeros}: L, M, C = {design}, K = {r.K}")
    cuts, state, out = H.piece_cuts(x.shape[1], r.K), None, []
    for a, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        res = r.run(x[:, lo:hi], state=state, flush=a == len(cuts) - 2)
        state = res.state
        out.append(res.y)
    assert np.array_equal(np.concatenate(out, axis=1), whole.y)


# ---- far stream positions -----------------------------------------------------------------------------------------------------------------

T = 3000
LIMIT = 1 << 40                                                                  # frt_resample_run: first_in + n <= 2^40


@functools.lru_cache(maxsize=None)
def far_case(rate):
    """(the default design of `rate`, a carried tail [S, K - 1], T samples)."""
    r = Resampler(rate)
    rng = np.random.default_rng(rate)
    return r, frozen(rng.standard_normal((S, r.K - 1))), frozen(rng.standard_normal((S, T)))


def far_positions(r):
    a = (LIMIT - T) // r.M
    return {"past-int32": (1 << 31) + 12345, "last-admissible": LIMIT - T, "whole-periods": a * r.M}


def run_at(rate, n_in):
    """The T samples behind the tail at stream position n_in, not flushed, then a flush without samples -> the outputs."""
    r, tail, x = far_case(rate)
    state = ResampleState(tail, n_in, r.n_out(n_in, False))
    first = r.run(x, state=state, flush=False)
    assert first.state.n_in == n_in + T and first.state.n_out == r.n_out(n_in + T, False)
    assert np.array_equal(first.state.tail, np.concatenate([tail, x], axis=1)[:, T:])
    rest = r.run(x[:, :0], state=first.state, flush=True)
    assert rest.state.n_out == r.n_out(n_in + T, True) and rest.y.shape[1] > 0
    y = np.concatenate([first.y, rest.y], axis=1)
    assert y.shape == (S, r.n_out(n_in + T, True) - state.n_out)
    return y


def check_at(rate, n_in, y):
    r, tail, x = far_case(rate)
    ref, B = H.reference_and_bound(np.concatenate([tail, x], axis=1), r.L, r.M, r.C, r.prototype, r.n_out(n_in, False),
                                   r.n_out(n_in + T, True), k0=n_in - (r.K - 1))
    within(y, ref, B, f"{rate} Hz at input {n_in}")


@pytest.mark.parametrize("where", ("past-int32", "last-admissible", "whole-periods"))
@pytest.mark.parametrize("rate", (44100, 3840000))
def test_far_stream_positions(hip, rate, where):
    r = far_case(rate)[0]
    n_in = far_positions(r)[where]
    assert (where == "whole-periods") == (n_in % r.M == 0) and n_in + T <= LIMIT and (where != "last-admissible" or n_in + T == LIMIT)
    y = run_at(rate, n_in)
    check_at(rate, n_in, y)
    if where == "whole-periods":
        # a shift by whole periods: the bits depend on the position within the period and on nothing else
        near = (-(-(r.K - 1) // r.M) + 1) * r.M
        assert LIMIT - T - r.M < n_in and r.K - 1 <= near < 1 << 20
        y_near = run_at(rate, near)
        check_at(rate, near, y_near)
        assert np.array_equal(y, y_near)


def test_a_position_past_the_limit_is_refused_and_nothing_is_written(hip):
    import torch
    r, tail, x = far_case(44100)
    n_in = LIMIT - T + 1
    with pytest.raises(_lib.FritureHipError, match="frt_resample_run: bad position"):
        r.run(x, state=ResampleState(tail, n_in, r.n_out(n_in, False)), flush=False)
    d = H.Device(r.L, r.M, r.C, r.prototype, S)
    try:
        first_out, n_out = r.n_out(n_in, False), 100
        for dev in (False, True):
            y, tail_out = np.full((S, n_out), SENTINEL), np.full((S, r.K - 1), SENTINEL)
            if dev:
                y, tail_out = torch.from_numpy(y).cuda(), torch.from_numpy(tail_out).cuda()
                torch.cuda.synchronize()
            ptr = (lambda a: a.data_ptr()) if dev else (lambda a: a.ctypes.data)
            rc = d.call(x.ctypes.data, 1, T, T, tail.ctypes.data, ptr(tail_out), n_in, first_out, n_out, ptr(y), 1, n_out)
            assert rc == -1 and "frt_resample_run: bad position" in d.last_error()
            if dev:
                torch.cuda.synchronize()
                y, tail_out = y.cpu().numpy(), tail_out.cpu().numpy()
            assert np.all(y == SENTINEL) and np.all(tail_out == SENTINEL)
        # the same call one sample earlier is the last admissible one
        y = np.full((S, n_out), SENTINEL)
        assert d.call(x.ctypes.data, 1, T - 1, T, tail.ctypes.data, None, n_in, first_out, n_out, y.ctypes.data, 1, n_out) == 0, d.last_error()
        assert not np.any(y == SENTINEL)
    finally:
        d.close()


# ---- layout arguments and extremes of the C entry point ----------------------------------------------------------------------------------

LAYOUT = (3, 2, 12)


@functools.lru_cache(maxsize=None)
def layout_case():
    """Three streams of the (3, 2, 12) row, cut once at input 100: (device, x, cut, the contiguous calls' outputs and states)."""
    d, x = device(*LAYOUT, streams=3), samples(*LAYOUT, streams=3)
    cuts = (0, 100, x.shape[1])
    out, states = d.pieces(x, cuts)
    ref, B = reference(*LAYOUT, streams=3)
    within(np.concatenate(out, axis=1), ref, B, "three streams, contiguous")
    return d, x, cuts, out, states


def padded_calls(make, ptr, read):
    """Both pieces of layout_case with ld = n + 5 and ldy = n_out + 3 and the payload one column in: the padding of x is NaN,
    the padding of y a sentinel.  make(array) -> a buffer the entry point takes, ptr(buffer, column) -> the address of [0, column],
    read(buffer) -> numpy."""
    d, x, cuts, out, states = layout_case()
    tail, first_out = None, 0
    for (lo, hi), want, (want_tail, _, total) in zip(zip(cuts[:-1], cuts[1:]), out, states):
        n, n_out = hi - lo, total - first_out
        assert n_out == want.shape[1] > 0
        xp, yp = np.full((3, n + 5), np.nan), np.full((3, n_out + 3), SENTINEL)
        xp[:, 1:1 + n] = x[:, lo:hi]
        xb, yb, tb = make(xp), make(yp), make(np.full((3, d.K - 1), SENTINEL))
        tin = None if tail is None else make(tail)
        rc = d.call(ptr(xb, 1), 1, n, n + 5, None if tin is None else ptr(tin, 0), ptr(tb, 0), lo, first_out, n_out, ptr(yb, 1), 1, n_out + 3)
        assert rc == 0, d.last_error()
        y, tail = read(yb), read(tb)
        assert np.array_equal(y[:, 1:1 + n_out], want)                            # bit for bit the contiguous call
        assert np.all(y[:, :1] == SENTINEL) and np.all(y[:, 1 + n_out:] == SENTINEL)
        assert np.array_equal(tail, want_tail)
        assert np.array_equal(read(xb), xp, equal_nan=True)
        first_out = total


def test_padded_rows_host_pointers(hip):
    padded_calls(lambda a: a, lambda a, col: a.ctypes.data + col * a.itemsize, lambda a: a)


def test_padded_rows_device_pointers(hip):
    import torch

    def make(a):
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        return t

    def read(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def ptr(t, col):
        view = t[:, col:]
        assert col == 0 or not view.is_contiguous()
        return view.data_ptr()

    padded_calls(make, ptr, read)


def test_the_most_streams(hip):
    L, M, C, streams, n = 5, 3, 3, 65535, 16
    x = np.random.default_rng(65535).standard_normal((streams, n))
    d = H.Device(L, M, C, prototype(C), streams)
    try:
        y, (tail, n_in, n_out) = d.run(x)
    finally:
        d.close()
    ref, B = H.reference_and_bound(x, L, M, C, prototype(C), 0, H.count(n, L, M, C, True))
    assert y.shape == ref.shape == (streams, 27) and (n_in, n_out) == (n, 27)
    within(y, ref, B, "65535 streams")
    assert np.array_equal(tail, x[:, n - 1:])
    alone = device(L, M, C, streams=1)
    for s in (0, 1, streams - 1):
        assert np.array_equal(alone.run(x[s:s + 1])[0], y[s:s + 1]), s


def test_calls_without_outputs_carry_the_tail_on_the_direct_path(hip):
    design = (601, 1499, 5996)
    d, x, K = device(*design), samples(*design), plan(*design)["K"]
    assert plan(*design)["direct"] and d.n_out(9, False) == 0 < d.n_out(10, False)
    cuts = (0, 4, 9, x.shape[1])
    out, states = d.pieces(x, cuts)
    assert out[0].shape == out[1].shape == (S, 0)
    tails_are_the_last_inputs(x, cuts, states, K)
    assert np.array_equal(np.concatenate(out, axis=1), d.run(x)[0])
