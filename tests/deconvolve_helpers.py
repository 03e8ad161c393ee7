"""The numpy restatement of X4 (include/friture_hip.h): the long real transform and deconvolution by regularised spectral
division, in float64 or in np.longdouble (numpy transforms longdouble natively: the yardstick of the GPU tests), the signals of
the tests and their distances.  Host only."""
import functools

import numpy as np

LD = np.longdouble
SPEC_BAR = 1e-12                            # max |X - X_ref| <= SPEC_BAR max |X_ref|: X1's bar
H_BAR = 1e-12                               # max |h - h_ref| <= H_BAR max |h_ref|
REF_BAR = 1e-13                             # numpy's float64 restatement against the longdouble one, asserted per parity case
FS = 48000


def padded(x, n, real=np.float64):
    """x [.., T <= n] continued with zeros to n, as `real`."""
    x = np.asarray(x)
    out = np.zeros(x.shape[:-1] + (n,), real)
    out[..., :x.shape[-1]] = x
    return out


def rfft(x, n, real=LD):
    return np.fft.rfft(padded(x, n, real), axis=-1)


def irfft(spec, n, keep=None):
    """numpy.fft.irfft(spec, n)[.., :keep] in the precision of spec."""
    return np.fft.irfft(spec, n, axis=-1)[..., :keep]


def inverse_spectrum(x, n, reg, real=LD):
    """G [refs, n/2 + 1] of the references x [refs, Lx] (or [Lx]): conj(X) / (P + r Pmax), 0 where the denominator is 0."""
    X = rfft(np.atleast_2d(x), n, real)
    P = X.real ** 2 + X.imag ** 2
    den = P + np.asarray(reg, real) * P.max(axis=-1, keepdims=True)
    ok = den != 0
    return np.where(ok, np.conj(X) / np.where(ok, den, 1), 0)


def restate(x, y, n, reg, keep=None, real=LD):
    """(h [S, keep], H [S, n/2 + 1]) of the measured rows y [S, T] against the references x ([Lx] or [S, Lx])."""
    H = rfft(np.atleast_2d(y), n, real) * inverse_spectrum(x, n, reg, real)
    return irfft(H, n, keep), H


def spectrum_bound(x, y, n, reg):
    """What the spectral bar allows on H = Y G per bin, [S, n/2 + 1] float64.  With |dX| <= e_x = SPEC_BAR max |X| and |dY| <= e_y =
    SPEC_BAR max |Y| on every bin, den = P + r Pmax and G = conj(X) / den: dG = conj(dX) / den - conj(X) dden / den^2 with |dden|
    <= 2 |X| e_x + 2 r max |X| e_x, and P / den <= 1, r Pmax / den <= 1 give |dG| <= 5 e_x / den; so |dH| <= |G| e_y + 5 |Y| e_x /
    den to first order.  Where den = 0 the bound is 0: H is exactly 0 there."""
    X, Y = rfft(np.atleast_2d(x), n), rfft(np.atleast_2d(y), n)
    P = X.real ** 2 + X.imag ** 2
    den = P + np.asarray(reg, LD) * P.max(axis=-1, keepdims=True)
    ok = den != 0
    safe = np.where(ok, den, 1)
    e_x, e_y = SPEC_BAR * np.abs(X).max(axis=-1, keepdims=True), SPEC_BAR * np.abs(Y).max(axis=-1, keepdims=True)
    return np.where(ok, np.abs(X) / safe * e_y + 5 * np.abs(Y) * e_x / safe, 0).astype(np.float64)


def distance(got, ref):
    """max |got - ref| / max |ref| (0 for two zero arrays), as a float."""
    ref = np.asarray(ref)
    top = np.abs(ref).max()
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref).max()
    return float(err / top) if top > 0 else float(err)


def exp_sweep(f0, f1, length, fs=FS, fade=0):
    """The sweep of friture_amd.deconvolve.exp_sweep, restated."""
    t = np.arange(length) / fs
    Td, K = length / fs, np.log(f1 / f0)
    x = np.sin(2 * np.pi * f0 * Td / K * (np.exp(t * K / Td) - 1))
    if fade:
        x[:fade] *= np.sin(np.linspace(0, np.pi / 2, fade)) ** 2
        x[length - fade:] *= np.cos(np.linspace(0, np.pi / 2, fade)) ** 2
    return x


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def response(seed, Lh, tau=None):
    """A decaying noise response [Lh]: what a room answers."""
    return noise(seed, Lh) * np.exp(-np.arange(Lh) / (tau or Lh / 8))


def band_reg(n, f_lo=20.0, f_hi=20000.0, inside=1e-8, outside=1e-2, fs=FS):
    """r [n/2 + 1]: `inside` on the bins of f_lo .. f_hi, `outside` elsewhere."""
    f = np.arange(n // 2 + 1) * (fs / n)
    return np.where((f >= f_lo) & (f <= f_hi), inside, outside)


@functools.lru_cache(maxsize=None)
def measurement(kind, Lx, rows, T, n, seed=0):
    """(x [Lx], y [rows, T]) shared by the parity cases: the reference (`kind`: "sweep" or "noise") through `rows` decaying
    responses (circularly at n, cut to T) plus a little noise; read-only."""
    x = exp_sweep(20.0, 20000.0, Lx, fade=Lx // 64) if kind == "sweep" else noise(seed + 1, Lx)
    X = np.fft.rfft(x, n)
    y = np.stack([np.fft.irfft(X * np.fft.rfft(response(seed + 10 + r, Lx // 2), n), n)[:T] for r in range(rows)])
    y += 1e-3 * noise(seed + 2, rows, T)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
