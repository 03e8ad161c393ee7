"""The resampler tests' numpy restatement of the definition in include/friture_hip.h (R1), in its gather form.  It designs
nothing: L, M, C and the prototype h are arguments, so the design tests do not depend on it.  The product does not import it."""
from __future__ import annotations

import numpy as np

RATES = (44100, 88200, 96000, 192000, 32000, 11025, 8000)
# rate -> (L, M, K) at the defaults (zeros 64, 48 kHz out); C = 64 max(L, M)
DESIGN = {44100: (160, 147, 129), 88200: (80, 147, 236), 96000: (1, 2, 257), 192000: (1, 4, 513), 32000: (3, 2, 129),
          11025: (640, 147, 129), 8000: (6, 1, 129)}
CUTS = (0, 1, 5, 300, 301, 650, 700)


def taps(L, C):
    return -(-(2 * C + 1) // L)


def count(n_in, L, M, C, flush):
    """Outputs after n_in inputs in total."""
    return -(-(n_in * L) // M) if flush else max(0, -(-(n_in * L - C) // M))


def gather(x, L, M, C, h, m0, m1, k0=0):
    """Outputs m0 .. m1 - 1 of the stream whose samples k0 .. k0 + x.shape[-1] - 1 are x [..., n] (zeros elsewhere):
    y[m] = sum_k h[C + m M - k L] x[k] over 0 <= C + m M - k L <= 2C, as index matrices k = kb(m) + j, i = C + m M - k L."""
    x = np.asarray(x, np.float64)
    K = taps(L, C)
    m = np.arange(m0, m1, dtype=np.int64)[:, None]
    kb = -(-(m * M - C) // L)
    k = kb + np.arange(K, dtype=np.int64)[None, :]
    i = C + m * M - k * L
    ok_i = (i >= 0) & (i <= 2 * C)
    ok_k = (k >= k0) & (k < k0 + x.shape[-1])
    hh = np.where(ok_i, h[np.clip(i, 0, 2 * C)], 0.0)
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1] + (m1 - m0,))
    xx = np.where(ok_k, x[..., np.clip(k - k0, 0, x.shape[-1] - 1)], 0.0)
    return np.sum(hh * xx, axis=-1)


def resample(x, L, M, C, h, flush=True):
    """The whole stream x [..., N] in one piece."""
    return gather(x, L, M, C, h, 0, count(x.shape[-1], L, M, C, flush))


def pieces(x, L, M, C, h, cuts):
    """x [N] cut at `cuts` (flush on the last piece only) with the carried-state bookkeeping replayed: per piece the outputs it
    emits, formed from the tail (the last K - 1 inputs, zeros before the start) and the piece alone.  Returns (list of output
    arrays, the smallest kb - (n_in - (K - 1)) seen: never negative when nothing reaches behind the tail)."""
    K = taps(L, C)
    tail, n_in, n_out, out, slack = np.zeros(K - 1), 0, 0, [], None
    for a, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        total = count(hi, L, M, C, a == len(cuts) - 2)
        buf = np.concatenate([tail, x[lo:hi]])
        if total > n_out:
            d = -(-(n_out * M - C) // L) - (n_in - (K - 1))
            slack = d if slack is None else min(slack, d)
        out.append(gather(buf, L, M, C, h, n_out, total, k0=n_in - (K - 1)))
        tail, n_in, n_out = buf[len(buf) - (K - 1):], hi, total
    return out, slack


def sine(rate, n=6000, f=1000.0, amp=0.5):
    return amp * np.sin(2 * np.pi * f * np.arange(n) / rate)


def sine_error(y, L, M, C, rate_out=48000, f=1000.0, amp=0.5):
    """max |y - the analytic sine at rate_out| away from the ends: the first and last ceil(2C / M) + 2 outputs are left out."""
    skip = -(-(2 * C) // M) + 2
    assert y.shape[-1] > 2 * skip + 16, "too few outputs away from the ends"
    ref = amp * np.sin(2 * np.pi * f * np.arange(y.shape[-1]) / rate_out)
    return float(np.max(np.abs(y - ref)[..., skip:y.shape[-1] - skip]))
