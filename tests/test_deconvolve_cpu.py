"""DeconvolveBatch without a GPU: the restatement of X4 (tests/deconvolve_helpers.py) against scipy.signal and np.fft, the host
helpers (exp_sweep, harmonic_offsets, the default n), the host side of friture_amd/deconvolve.py and the argument checks of the C
entry points that precede any device call."""
import ctypes
import math

import numpy as np
import pytest

import deconvolve_helpers as dh
from friture_amd import deconvolve as dc


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def test_the_restatement_recovers_a_response_that_scipy_applied():
    import scipy.signal
    x, h = dh.noise(1, 300), dh.response(2, 100)
    y = scipy.signal.fftconvolve(x, h)[None]
    got, H = dh.restate(x, y, 1 << 13, 0.0, keep=100, real=np.float64)
    d = dh.distance(got[0], h)
    print(f"float64 restatement against the applied response: {d:.2e}")
    assert got.shape == (1, 100) and H.shape == (1, 4097) and d <= 1e-9
    assert np.array_equal(dh.rfft(x, 1 << 13, np.float64), np.fft.rfft(x, 1 << 13))
    assert dh.rfft(x, 1 << 13).dtype == np.result_type(np.longdouble, np.complex64)
    d = dh.distance(np.fft.rfft(x, 1 << 13), dh.rfft(x, 1 << 13))
    print(f"np.fft.rfft in float64 against longdouble: {d:.2e}")
    assert d <= 1e-15 < dh.SPEC_BAR


def test_regularisation_and_zero_denominators():
    n = 1 << 13
    x = np.tile([1.0, 0.0, -1.0, 0.0], n // 4)                   # one live bin, n / 4
    G = dh.inverse_spectrum(x, n, 0.0, np.float64)[0]
    P = np.abs(np.fft.rfft(x)) ** 2
    assert np.all(G[P == 0] == 0) and np.count_nonzero(P == 0) > 0 and np.all(np.isfinite(G))
    assert abs(G[n // 4] - 2.0 / n) <= 1e-15
    G = dh.inverse_spectrum(dh.noise(3, 500), n, dh.band_reg(n), np.float64)
    X = np.fft.rfft(dh.noise(3, 500), n)
    P = np.abs(X) ** 2
    assert np.allclose(G[0], np.conj(X) / (P + dh.band_reg(n) * P.max()), rtol=1e-12, atol=0)
    r = dh.band_reg(n)
    assert r[0] == 1e-2 and r[n // 2] == 1e-2 and r[n // 8] == 1e-8


@pytest.mark.parametrize("kind, reg", [("sweep", 1e-6), ("noise", 0.0)])
def test_float64_and_longdouble_restatements_agree_far_inside_the_bar(kind, reg):
    n = 1 << 14
    x, y = dh.measurement(kind, 1 << 12, 2, (1 << 13) + 5, n)
    d = dh.distance(dh.restate(x, y, n, reg, real=np.float64)[0], dh.restate(x, y, n, reg)[0])
    print(f"{kind}, reg {reg}: float64 against longdouble {d:.2e}")
    assert d <= dh.REF_BAR < dh.H_BAR


# ---- the host helpers -----------------------------------------------------------------------------------------------------------

def test_exp_sweep_follows_its_definition():
    L, f0, f1 = 1 << 14, 50.0, 5000.0
    x = dc.exp_sweep(f0, f1, L)
    assert x.dtype == np.float64 and x.shape == (L,) and x[0] == 0.0
    assert np.allclose(x, dh.exp_sweep(f0, f1, L), rtol=0, atol=1e-9)
    # the instantaneous frequency f0 exp(t K / Td) at both ends, from the phase of the definition
    Td, K = L / dh.FS, math.log(f1 / f0)
    phase = 2 * np.pi * f0 * Td / K * np.expm1(np.arange(L + 1) / dh.FS * K / Td)
    inst = np.diff(phase) * dh.FS / (2 * np.pi)
    assert abs(inst[0] / f0 - 1) <= 1e-3 and abs(inst[-1] / f1 - 1) <= 1e-3
    assert np.allclose(x[:64], np.sin(phase[:64]), rtol=0, atol=1e-12)
    f = dc.exp_sweep(f0, f1, L, fade=100)
    assert np.array_equal(f[100:L - 100], x[100:L - 100]) and f[0] == 0.0 and abs(f[-1]) <= 1e-12
    assert np.allclose(f, dh.exp_sweep(f0, f1, L, fade=100), rtol=0, atol=1e-9)
    assert np.all(np.abs(f[:100]) <= np.abs(x[:100]) + 1e-15)
    for bad in (dict(f0=0.0), dict(f1=30000.0), dict(f0=6000.0), dict(length=1), dict(length=2.5), dict(fade=-1), dict(fade=L), dict(fs=0)):
        with pytest.raises(ValueError):
            dc.exp_sweep(**{**dict(f0=f0, f1=f1, length=L), **bad})


def test_harmonic_offsets_are_the_closed_form():
    off = dc.harmonic_offsets(1 << 18, 20.0, 20000.0, orders=(2, 3))
    assert off.dtype == np.float64 and np.allclose(off, [(1 << 18) * math.log(k) / math.log(1000.0) for k in (2, 3)], rtol=1e-15)
    assert dc.harmonic_offsets(1000, 20.0, 200.0, orders=(1,))[0] == 0.0
    assert np.allclose(dc.harmonic_offsets(1000, 20.0, 200.0, orders=[10]), [1000.0])
    for bad in (dict(orders=(0,)), dict(orders=(1.5,)), dict(f0=0.0), dict(f1=10.0), dict(sweep_len=0)):
        with pytest.raises(ValueError):
            dc.harmonic_offsets(**{**dict(sweep_len=1000, f0=20.0, f1=200.0), **bad})


def test_default_n():
    for Lx, n in ((1, 1 << 13), (4096, 1 << 13), (4097, 1 << 14), (1 << 18, 1 << 19), ((1 << 18) + 1, 1 << 20), (1 << 23, 1 << 24)):
        assert dc.default_n(Lx) == n == dc.DeconvolveBatch(np.ones(Lx)).n
    assert dc.DeconvolveBatch(np.ones((1 << 23) + 1), n=1 << 24).n == 1 << 24
    with pytest.raises(ValueError, match="give n"):
        dc.DeconvolveBatch(np.ones((1 << 23) + 1))
    b = dc.DeconvolveBatch([[1, 2, 3], [4, 5, 6]], reg=0)
    assert (b.refs, b.Lx, b.n, b.per_row, b.reg, b.reg_bins) == (2, 3, 1 << 13, True, 0.0, None) and b.ref.dtype == np.float64
    b = dc.DeconvolveBatch(np.ones(5), reg=dh.band_reg(1 << 13))
    assert b.reg_bins.shape == (4097,) and not b.per_row


# ---- the host side --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("x, kwargs", [(np.ones(0), {}), (np.ones((1, 2, 3)), {}), (np.ones(4, complex), {}), (np.array([1.0, np.nan]), {}),
                                       (np.array([1.0, np.inf]), {}), (np.ones(4), dict(n=1 << 12)), (np.ones(4), dict(n=1 << 25)),
                                       (np.ones(4), dict(n=3 << 12)), (np.ones(4), dict(n=8192.0)), (np.ones(4), dict(n=True)),
                                       (np.ones(8193), dict(n=8192)), (np.ones(4), dict(reg=-1e-9)), (np.ones(4), dict(reg=np.nan)),
                                       (np.ones(4), dict(reg=np.inf)), (np.ones(4), dict(reg=np.ones(4096))), (np.ones(4), dict(reg=-np.ones(4097))),
                                       (np.ones(4), dict(reg=np.ones(4097, complex))), (np.ones(4), dict(reg="1e-6"))])
def test_argument_errors(x, kwargs):
    with pytest.raises(ValueError):
        dc.DeconvolveBatch(x, **kwargs)


def test_input_errors_precede_the_device():
    b = dc.DeconvolveBatch(np.ones((2, 5)))
    with pytest.raises(TypeError):
        b.run([[0.0] * 64] * 2)
    with pytest.raises(TypeError):
        b.run(np.zeros((2, 64), np.int16))
    with pytest.raises(ValueError):
        b.run(np.zeros((1, 2, 64)))
    with pytest.raises(ValueError, match="references"):
        b.run(np.zeros((3, 64)))
    with pytest.raises(ValueError, match="samples per row"):
        b.run(np.zeros((2, 8193)))
    with pytest.raises(ValueError, match="samples per row"):
        b.run(np.zeros((2, 0)))
    with pytest.raises(ValueError):
        b.run(np.zeros((2, 64)), scratch_bytes=-1)
    for keep in (0, 8193, 2.0, True):
        with pytest.raises(ValueError, match="keep"):
            b.run(np.zeros((2, 64)), keep=keep)
    with pytest.raises(TypeError):
        dc.rfft_rows([0.0] * 64, 1 << 13)
    with pytest.raises(TypeError):
        dc.rfft_rows(np.zeros(64, np.int32), 1 << 13)
    for n in (1 << 12, 1 << 25, 10000, 8192.0):
        with pytest.raises(ValueError):
            dc.rfft_rows(np.zeros(64), n)
    with pytest.raises(ValueError):
        dc.rfft_rows(np.zeros(8193), 1 << 13)
    with pytest.raises(ValueError):
        dc.rfft_rows(np.zeros((2, 0)), 1 << 13)
    with pytest.raises(ValueError):
        dc.rfft_rows(np.zeros(64), 1 << 13, scratch_bytes=-1)
    with pytest.raises(TypeError):
        dc.irfft_rows(np.zeros((2, 4097)), 1 << 13)
    with pytest.raises(TypeError):
        dc.irfft_rows([0j] * 4097, 1 << 13)
    with pytest.raises(ValueError):
        dc.irfft_rows(np.zeros((2, 4096), complex), 1 << 13)
    with pytest.raises(ValueError):
        dc.irfft_rows(np.zeros((2, 4097), complex), 1 << 12)
    for keep in (0, 8193, 1.5):
        with pytest.raises(ValueError, match="keep"):
            dc.irfft_rows(np.zeros((2, 4097), complex), 1 << 13, keep=keep)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_reject_bad_arguments_before_any_device_call():
    from friture_amd import _lib
    lib = _lib.load()
    for name in ("frt_rfft_long_rows", "frt_irfft_long_rows", "frt_deconvolve_create", "frt_deconvolve_destroy", "frt_deconvolve_set_stream",
                 "frt_deconvolve_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    N = 1 << 13
    t = np.ones(N)
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bad = np.ones(N)
    bad[7] = np.nan
    bp = bad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    neg = np.ones(N // 2 + 1)
    neg[9] = -1.0
    np_ = neg.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    # frt_deconvolve_create(&h, x, Lx, refs, n, reg, reg_bins)
    for args, status, word in (((None, 4, 1, N, 0.0, None), -1, b"null reference"), ((tp, 0, 1, N, 0.0, None), -1, b"Lx 0"),
                               ((tp, N + 1, 1, N, 0.0, None), -1, b"Lx 8193"), ((tp, 4, 1, N // 2, 0.0, None), -1, b"n 4096"),
                               ((tp, 4, 1, 1 << 25, 0.0, None), -1, b"n 33554432"), ((tp, 4, 1, 3 << 12, 0.0, None), -1, b"n 12288"),
                               ((tp, 4, 0, N, 0.0, None), -1, b"references"), ((tp, 4, 65536, N, 0.0, None), -1, b"references"),
                               ((tp, 4, 1, N, -1e-9, None), -1, b"reg"), ((tp, 4, 1, N, math.nan, None), -1, b"reg"),
                               ((tp, 4, 1, N, math.inf, None), -1, b"reg"), ((bp, 8, 1, N, 0.0, None), -1, b"x[7] is not finite"),
                               ((tp, 4, 1, N, 0.0, np_), -1, b"reg_bins[9]"), ((tp, 4, 9, 1 << 24, 0.0, None), -4, b"not supported")):
        h = ctypes.c_void_p()
        assert lib.frt_deconvolve_create(ctypes.byref(h), *args) == status and h.value is None, args[1:]
        assert b"frt_deconvolve_create" in lib.frt_last_error() and word in lib.frt_last_error(), lib.frt_last_error()
    assert lib.frt_deconvolve_create(None, tp, 4, 1, N, 0.0, None) == -1
    assert lib.frt_deconvolve_run(None, None, 0, 1, 1, 1, 1, 0, None, 1, None) == -1 and b"frt_deconvolve_run" in lib.frt_last_error()
    assert lib.frt_deconvolve_set_stream(None, None) == -1
    lib.frt_deconvolve_destroy(None)
    vp = ctypes.c_void_p
    x, spec = vp(t.ctypes.data), vp(np.zeros(2 * (N // 2 + 1)).ctypes.data)
    # frt_rfft_long_rows(x, x_dtype, rows, T, row_stride, n, scratch_bytes, spec, stream)
    for args, word in (((None, 1, 1, 4, 4, N, 0, spec, None), b"null buffer"), ((x, 1, 1, 4, 4, N, 0, None, None), b"null buffer"),
                       ((x, 2, 1, 4, 4, N, 0, spec, None), b"x_dtype 2"), ((x, 1, 1, 4, 4, N // 2, 0, spec, None), b"n 4096"),
                       ((x, 1, 1, 4, 4, 1 << 25, 0, spec, None), b"n 33554432"), ((x, 1, 1, 4, 4, N + 8, 0, spec, None), b"n 8200"),
                       ((x, 1, 1, 0, 4, N, 0, spec, None), b"T 0"), ((x, 1, 1, N + 1, N + 1, N, 0, spec, None), b"T 8193"),
                       ((x, 1, 0, 4, 4, N, 0, spec, None), b"rows"), ((x, 1, 65536, 4, 4, N, 0, spec, None), b"rows"),
                       ((x, 1, 2, 4, 3, N, 0, spec, None), b"bad stride"), ((x, 1, 1, 4, 4, N, -1, spec, None), b"scratch_bytes")):
        assert lib.frt_rfft_long_rows(*args) == -1, args[1:]
        assert b"frt_rfft_long_rows" in lib.frt_last_error() and word in lib.frt_last_error(), lib.frt_last_error()
    # frt_irfft_long_rows(spec, rows, n, keep, scratch_bytes, out, out_stride, stream)
    for args, word in (((None, 1, N, 4, 0, x, 4, None), b"null buffer"), ((spec, 1, N, 4, 0, None, 4, None), b"null buffer"),
                       ((spec, 1, N // 2, 4, 0, x, 4, None), b"n 4096"), ((spec, 1, 10000, 4, 0, x, 4, None), b"n 10000"),
                       ((spec, 1, N, 0, 0, x, 4, None), b"keep 0"), ((spec, 1, N, N + 1, 0, x, N + 1, None), b"keep 8193"),
                       ((spec, 0, N, 4, 0, x, 4, None), b"rows"), ((spec, 65536, N, 4, 0, x, 4, None), b"rows"),
                       ((spec, 2, N, 4, 0, x, 3, None), b"bad stride"), ((spec, 1, N, 4, -1, x, 4, None), b"scratch_bytes")):
        assert lib.frt_irfft_long_rows(*args) == -1, args[1:]
        assert b"frt_irfft_long_rows" in lib.frt_last_error() and word in lib.frt_last_error(), lib.frt_last_error()


def test_impulse_response_keeps_its_range():
    from friture_amd import convolve as cv
    assert (cv.MIN_IRFFT, cv.MAX_IRFFT) == (64, 8192) and dc.MIN_N == 1 << 13 and dc.MAX_N == 1 << 24
