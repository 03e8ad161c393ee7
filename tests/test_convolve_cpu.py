"""ConvolveBatch without a GPU: the restatement of X2 (tests/convolve_helpers.py) against itself, the emitted counts, the state
layout, the host side of friture_amd/convolve.py (arguments, the state's rejections) and the argument checks of the C entry
points that precede any device call."""
import ctypes

import numpy as np
import pytest

import convolve_helpers as ch
from friture_amd import convolve as cv


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def test_a_delta_gives_the_taps_and_convolution_commutes():
    h = ch.taps(1, 37)
    delta = np.zeros(20)
    delta[3] = 1.0
    y = ch.restate(delta, h)
    assert y.shape == (1, 56) and np.array_equal(y[0, 3:40], h) and not y[0, :3].any() and not y[0, 40:].any()
    x = ch.signal(2, 1, 50)
    assert np.allclose(ch.restate(x, h), ch.restate(h, x[0]), rtol=0, atol=1e-14)
    assert np.array_equal(ch.restate_long(delta, h)[0, 3:40], h.astype(np.longdouble))


def test_float64_and_longdouble_restatements_agree_far_inside_the_bar():
    x, h = ch.signal(3, 2, 300), ch.taps(3, 70, 2)
    d = ch.distance(ch.restate(x, h), x, h, ch.restate_long(x, h))
    print(f"np.convolve against the longdouble sum: {d:.2e}")
    assert d <= 1e-15 < ch.BAR
    assert ch.distance(np.zeros((1, 12)), np.zeros((1, 10)), np.ones(3)) == 0.0


# ---- counts and the state layout ------------------------------------------------------------------------------------------------

def test_defaults_and_partitions():
    for L, block, P in ((1, 64, 1), (64, 64, 1), (65, 128, 1), (4096, 4096, 1), (4097, 4096, 2), (65536, 4096, 16), (1 << 18, 4096, 64)):
        b = cv.ConvolveBatch(np.ones(L))
        assert (b.L, b.block, b.partitions) == (L, block, P) and ch.default_block(L) == block == cv.default_block(L)
    b = cv.ConvolveBatch(np.ones((3, 200)), block=64)
    assert (b.L, b.block, b.partitions, b.filters, b.per_stream) == (200, 64, 4, 3, True)
    assert cv.ConvolveBatch([1, 2, 3]).taps.dtype == np.float64


def test_emitted_after():
    b = cv.ConvolveBatch(np.ones(70), block=64)
    for n in (0, 1, 63, 64, 65, 127, 128, 1000):
        assert b.emitted_after(n) == (n // 64) * 64 == ch.emitted_after(n, 70, 64)
        assert b.emitted_after(n, flushed=True) == n + 69 == ch.emitted_after(n, 70, 64, True)


@pytest.mark.parametrize("L, P", [(64, 1), (65, 2), (300, 5)])
def test_state_layout(L, P):
    B = 64
    b = cv.ConvolveBatch(np.ones(L), block=B)
    assert b.partitions == P
    for m in (0, 1, P, P + 1, P + 3):
        for n in (m * B - 1, m * B, m * B + 1, m * B + B - 1):
            if n < 0:
                continue
            start = max(0, (n // B - P) * B)
            assert cv.state_start(n, B, P) == ch.state_start(n, L, B) == start
            assert b.state_length(n) == n - start <= (P + 1) * B - 1
            x = ch.signal(4, 2, n)
            assert np.array_equal(ch.state_after(x, L, B), x[:, start:])


# ---- the host side --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h, kwargs", [(np.ones(0), {}), (np.ones((1, 2, 3)), {}), (np.ones((1 << 18) + 1), {}), (np.array([1.0, np.nan]), {}),
                                       (np.array([1.0, np.inf]), {}), (np.ones(4, complex), {}), (np.ones(4), dict(block=32)),
                                       (np.ones(4), dict(block=96)), (np.ones(4), dict(block=8192)), (np.ones(4), dict(block=64.0)),
                                       (np.ones(1 << 18), dict(block=32)), (np.ones((1 << 18)), dict(block=True))])
def test_argument_errors(h, kwargs):
    with pytest.raises(ValueError):
        cv.ConvolveBatch(h, **kwargs)


def test_input_errors_precede_the_device():
    b = cv.ConvolveBatch(np.ones((2, 5)))
    with pytest.raises(TypeError):
        b.run([[0.0] * 64] * 2)
    with pytest.raises(TypeError):
        b.run(np.zeros((2, 64), np.int16))
    with pytest.raises(ValueError):
        b.run(np.zeros((1, 2, 64)))
    with pytest.raises(ValueError, match="filters"):
        b.run(np.zeros((3, 64)))
    with pytest.raises(ValueError):
        b.run(np.zeros((2, 64)), scratch_bytes=-1)
    with pytest.raises(TypeError):
        b.run(np.zeros((2, 64)), dtype=np.int16)
    with pytest.raises(TypeError):
        cv.impulse_response(np.zeros((2, 33)))
    with pytest.raises(ValueError):
        cv.impulse_response(np.zeros((2, 30), complex))
    with pytest.raises(ValueError):
        cv.impulse_response(np.zeros((2, 8193), complex))


def state_of(b, S, n):
    return cv.ConvolveState(np.zeros((S, b.state_length(n))), S, n, b.emitted_after(n), b.settings)


def test_state_errors_precede_the_device():
    h = ch.taps(5, 70)
    b = cv.ConvolveBatch(h, block=64)
    good = state_of(b, 2, 200)
    x = np.zeros((2, 10))
    for other in (cv.ConvolveBatch(h, block=128), cv.ConvolveBatch(h[:69], block=64), cv.ConvolveBatch(h * 2, block=64),
                  cv.ConvolveBatch(np.stack([h, h]), block=64)):
        with pytest.raises(ValueError, match="other settings"):
            other.run(x, good)
    with pytest.raises(ValueError, match="another shape"):
        b.run(np.zeros((3, 10)), good)
    with pytest.raises(ValueError, match="another shape"):
        b.run(x, good._replace(tail=good.tail[:, :-1]))
    with pytest.raises(ValueError, match="another stream"):
        b.run(x, good._replace(n_out=good.n_out + 1))
    with pytest.raises(ValueError, match="another stream"):
        b.run(x, good._replace(n_in=-1))
    with pytest.raises(ValueError, match="flushed"):
        b.run(x, cv.ConvolveState(None, 2, 200, 269, b.settings))


# ---- the C entry points ---------------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_reject_bad_arguments_before_any_device_call():
    from friture_amd import _lib
    lib = _lib.load()
    for name in ("frt_convolve_create", "frt_convolve_destroy", "frt_convolve_set_stream", "frt_convolve_state_length", "frt_convolve_run",
                 "frt_irfft_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    t = np.ones(1 << 18)
    t[7] = np.nan
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for args, status, word in (((None, 4, 1, 0), -1, b"null taps"), ((tp, 0, 1, 0), -1, b"L 0"), ((tp, (1 << 18) + 1, 1, 0), -1, b"L 262145"),
                               ((tp, 4, 0, 0), -1, b"filters"), ((tp, 4, 1, 32), -1, b"block 32"), ((tp, 4, 1, 100), -1, b"block 100"),
                               ((tp, 4, 1, 8192), -1, b"block 8192"), ((tp, 1 << 18, 1, 32), -1, b"block 32"),
                               ((tp, 1 << 18, 1, 0), -1, b"taps[7] is not finite"), ((tp, 8, 1, 64), -1, b"not finite"),
                               ((tp, 1 << 18, 65535, 4096), -4, b"not supported")):
        h = ctypes.c_void_p()
        assert lib.frt_convolve_create(ctypes.byref(h), *args) == status and h.value is None, args[1:]
        assert b"frt_convolve_create" in lib.frt_last_error() and word in lib.frt_last_error(), lib.frt_last_error()
    assert lib.frt_convolve_create(None, tp, 4, 1, 0) == -1
    assert lib.frt_convolve_run(None, None, 0, 1, 0, 0, None, None, 0, 1, 0, None, 0, 0, None) == -1
    assert b"frt_convolve_run" in lib.frt_last_error()
    assert lib.frt_convolve_set_stream(None, None) == -1
    assert lib.frt_convolve_state_length(None, 1, 0) < 0
    lib.frt_convolve_destroy(None)
    for n in (32, 100, 16384):
        assert lib.frt_irfft_rows(None, 1, n, None, None) == -1 and b"frt_irfft_rows" in lib.frt_last_error()
    assert lib.frt_irfft_rows(None, 1, 64, None, None) == -1 and b"null buffer" in lib.frt_last_error()


def test_the_longest_filter_in_the_smallest_block_meets_the_partition_limit():
    assert cv.ConvolveBatch(np.ones(1 << 18), block=64).partitions == 4096 == cv.MAX_PARTITIONS
