"""The resampler tests' numpy restatement of the definition in include/friture_hip.h (R1), in its gather form.  It designs
nothing: L, M, C and the prototype h are arguments, so the design tests do not depend on it.  The product does not import it.
Also here: the same definition in extended precision with the a-priori rounding bound of the kernel's fma chain
(reference_and_bound), a restatement of frt_resample_create's launch planner with the table of designs that reach each of its
classes (launch_plan, ROWS), and a ctypes driver over the C entry points for any prototype and layout (Device)."""
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


# ---- the extended-precision reference and the a-priori rounding bound ---------------------------------------------------------------

EXTENDED = np.finfo(np.longdouble).nmant >= 63          # an 80-bit (or wider) long double; otherwise exact rationals


def extended(a, exact=None):
    """A float array in the precision of the reference, every value carried over exactly: np.longdouble where that has at least
    64 significant bits, otherwise (or with exact=True) an object array of fractions.Fraction.  Never float64."""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    if EXTENDED and not exact:
        return a.astype(np.longdouble)
    from fractions import Fraction
    out = np.empty(a.shape, object)
    out.ravel()[:] = [Fraction(float(v)) for v in a.ravel()]
    return out


def reference_and_bound(x, L, M, C, h, m0, m1, k0=0, exact=None):
    """(ref, B), each [..., m1 - m0] in the precision of `extended`: ref the outputs m0 .. m1 - 1 that `gather` defines, from
    float64 x [..., n] and h [2C + 1]; B[m] = gamma_K sum_j |h[i_j]| |x[k_j]|, gamma_K = K u / (1 - K u), u = 2^-53: the bound
    on |fl(y[m]) - y[m]| of ONE chain acc = fma(c, x, acc) over the K taps in any order (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., section 3.1 with one rounding per term), which is what the kernel promises.  A float32
    recording is passed as the float64 array of its values."""
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == np.float64 and h.dtype == np.float64 and h.shape == (2 * C + 1,)
    K, n = taps(L, C), x.shape[-1]
    xe, he = extended(x, exact), extended(h, exact)
    one = extended(np.ones(1), exact)[0]
    zero, u = one - one, one / 2 ** 53
    gamma = K * u / (one - K * u)
    ref = np.full(x.shape[:-1] + (m1 - m0,), zero, xe.dtype)
    B = ref.copy()
    if n == 0:
        return ref, B
    step = max(1, (1 << 20) // (K * max(1, x.size // n)))                       # outputs per block: bounded temporaries
    for a in range(m0, m1, step):
        m = np.arange(a, min(m1, a + step), dtype=np.int64)[:, None]
        k = -(-(m * M - C) // L) + np.arange(K, dtype=np.int64)[None, :]
        i = C + m * M - k * L
        ok = (i >= 0) & (i <= 2 * C) & (k >= k0) & (k < k0 + n)
        prod = np.where(ok, he[np.clip(i, 0, 2 * C)] * xe[..., np.clip(k - k0, 0, n - 1)], zero)
        ref[..., a - m0:a - m0 + len(m)] = prod.sum(axis=-1)
        B[..., a - m0:a - m0 + len(m)] = gamma * np.abs(prod).sum(axis=-1)
    return ref, B


def excess(y, ref, B, exact=None):
    """max over the outputs of |y - ref| / tolerance, in the precision of the reference; at most 1 when y is within the bound.
    float64 y: tolerance B.  float32 y: B + 2^-24 (|ref| + B), one more rounding of a float64 sum that is within B of ref.
    An output whose tolerance is 0 (every product is 0) must be exact: it counts as 0 or infinity."""
    assert y.dtype in (np.float32, np.float64) and y.shape == ref.shape == B.shape, (y.dtype, y.shape, ref.shape)
    err = np.abs(extended(y, exact) - ref)
    tol = B if y.dtype == np.float64 else B + (np.abs(ref) + B) / 2 ** 24
    pos = np.asarray(tol > 0, bool)
    if np.any(err[~pos] != 0):
        return np.inf
    return float(np.max(err[pos] / tol[pos])) if np.any(pos) else 0.0


# ---- the launch planner of frt_resample_create, restated --------------------------------------------------------------------------

def launch_plan(L, M, C, periods, tap_block, cap):
    """What frt_resample_create decides for (L, M, C) given resample.hip's kPeriods, kTapBlock and kCap, and which branches of
    resample_kernel the design then takes: K; dq = kb(L - 1) - kb(0); np, the periods side by side in a workgroup; direct
    (no tile fits LDS: samples are read from memory); span, the LDS slots of one copy; items = np L with the passes of the
    `it` loop, the threads of a workgroup and the items of the last pass; Kq, the set of per-column tap counts; blocks, the
    whole tap blocks of the `j + kTapBlock < K` loop; parities, the set of (first tap's LDS index) & 1 over every thread and
    period of a tile ({0, 1}: both LDS copies are read; empty on the direct path)."""
    ceil = lambda a, b: -(-a // b)
    kb = lambda q: ceil(q * M - C, L)
    K = (2 * C + L) // L
    dq = kb(L - 1) - kb(0)
    want, room = (256 + L - 1) // L, (cap // 2 - 2) - K - dq
    fit = 0 if room < 0 else (room // M + 1) // periods
    direct = fit < 1
    n_p = want if direct else min(want, fit)
    span = 0 if direct else (periods * n_p - 1) * M + dq + K
    items = n_p * L
    passes = ceil(items, 512)
    threads = ceil(ceil(items, passes), 64) * 64
    Kq = {(C + q * M - kb(q) * L) // L + 1 for q in range(L)}
    parities = set() if direct else {(kb(q) - kb(0) + (pt + r * n_p) * M) & 1 for q in range(L) for pt in range(n_p) for r in range(periods)}
    return dict(K=K, dq=dq, np=n_p, direct=direct, span=span, items=items, passes=passes, threads=threads,
                last=items - (passes - 1) * threads, Kq=Kq, blocks=max(0, (K - 1) // tap_block), parities=parities)


def kernel_constants(text):
    """(kPeriods, kTapBlock, kCap) as resample.hip declares them."""
    import re
    found = {name: int(v) for name, v in re.findall(r"constexpr\s+int\s+(kPeriods|kTapBlock|kCap)\s*=\s*(\d+)\s*;", text)}
    assert set(found) == {"kPeriods", "kTapBlock", "kCap"}, f"resample.hip declares {sorted(found)}"
    return found["kPeriods"], found["kTapBlock"], found["kCap"]


# (L, M, C) -> the branch class the design is in the table to reach, as the entries of launch_plan it must show.  The design
# tests of the GPU suite run these rows; test_resample_cpu.py holds them to the constants resample.hip has today.
ROWS = (
    ((5, 3, 3), dict(K=2, Kq={1, 2}, blocks=0, direct=False)),                      # minimum K: a tail of one sample
    ((3, 2, 3), dict(K=3, Kq={2, 3}, blocks=0, np=86, direct=False)),               # K <= kTapBlock, a column short of a tap
    ((3, 2, 4), dict(K=3, Kq={3}, blocks=0, direct=False)),                         # C no multiple of L: every column has K taps
    ((3, 2, 11), dict(K=8, blocks=0, direct=False)),                                # K = kTapBlock: the block loop still empty
    ((3, 2, 12), dict(K=9, Kq={8, 9}, blocks=1, direct=False)),                     # one block, then one tap or none
    ((2, 3, 15), dict(K=16, Kq={15, 16}, blocks=1, np=128, direct=False)),          # K = 2 kTapBlock: one block, then 7 or 8 taps
    ((1, 3, 12), dict(K=25, parities={0, 1}, direct=False)),                        # L = 1, M odd: both LDS copies are read
    ((160, 147, 300), dict(K=4, np=2, span=1179, direct=False)),                    # LDS holds fewer periods than 256 threads want
    ((1000, 3, 4000), dict(K=9, direct=False, passes=2, threads=512, last=488)),    # L > 512 in LDS, a ragged last pass
    ((1025, 2, 8200), dict(K=17, direct=False, passes=3, threads=384, last=257)),   # L just past a multiple of the block size
    ((601, 1499, 5996), dict(K=20, direct=True, passes=2)),                         # direct with L > 1
    ((2048, 2049, 8196), dict(K=9, direct=True, passes=4, threads=512, last=512)),  # direct, four full passes
    ((48000, 22051, 384000), dict(K=17, direct=True, passes=94, items=48000)),      # L K = 816 000 of 2^20 coefficients
)


def row_length(L, M, n_p, periods):
    """Inputs whose flushed outputs fill two tiles of `periods * n_p` periods and one period of a third (a period of L outputs
    advances the input by M samples), at least 37; plus the first of 3, 4, 5 more that leave the last period ragged too."""
    base = max(37, (2 * periods * n_p + 1) * M)
    return next(base + e for e in (3, 4, 5) if L == 1 or count(base + e, L, M, 0, True) % L)


def piece_cuts(n, K):
    """Cut points of n inputs into pieces of 0, 1, 2, K - 2, K - 1, K samples and the rest, clipped to what exists: the carried
    tail is then formed from the old tail alone, from part of it and new samples, and from new samples alone."""
    cuts = [0]
    for d in (0, 1, 2, K - 2, K - 1, K):
        cuts.append(min(n, cuts[-1] + d))
    return tuple(cuts) + (n,)


# ---- the C entry points, driven directly ------------------------------------------------------------------------------------------------

class Device:
    """frt_resample_create / run / destroy for any (L, M, C), any prototype h [2C + 1] and S streams.  call() passes raw
    addresses (host or device) and every layout argument through and returns the status; run() is the contiguous host-array
    call with the carried state (tail [S, K - 1], n_in, n_out) of a stream that started anywhere."""

    def __init__(self, L, M, C, h, S):
        import ctypes
        from friture_amd import _lib
        self.L, self.M, self.C, self.S, self.K = L, M, C, S, taps(L, C)
        self.h = np.ascontiguousarray(h, np.float64)
        assert self.h.shape == (2 * C + 1,)
        self._check, self.lib, self.handle = _lib.check, _lib.init(), ctypes.c_void_p()
        _lib.check(self.lib.frt_resample_create(ctypes.byref(self.handle), L, M, C,
                                                self.h.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), S))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.frt_resample_destroy(self.handle)
            self.handle.value = None

    __del__ = close

    def last_error(self):
        return self.lib.frt_last_error().decode(errors="replace")

    def call(self, x, x_code, n, ld, tail_in, tail_out, first_in, first_out, n_out, y, y_code, ldy):
        """frt_resample_run with addresses (or None) for x, tail_in, tail_out, y; codes: 0 float32, 1 float64."""
        assert self.handle.value, "closed"
        return self.lib.frt_resample_run(self.handle, x, x_code, n, ld, tail_in, tail_out, first_in, first_out, n_out, y, y_code, ldy)

    def n_out(self, n_in, flush=True):
        return count(n_in, self.L, self.M, self.C, flush)

    def run(self, x, state=None, flush=True, out=np.float64):
        """x [S, n] float32 or float64 on the host -> (y [S, n_new] of dtype `out`, the state after the call)."""
        tail, n_in, done = state if state is not None else (None, 0, 0)
        x = np.ascontiguousarray(x)
        assert x.shape[0] == self.S and x.dtype in (np.float32, np.float64)
        n = x.shape[1]
        total = self.n_out(n_in + n, flush)
        y, tail_out = np.full((self.S, total - done), np.nan, out), np.full((self.S, self.K - 1), np.nan)
        tail = None if tail is None else np.ascontiguousarray(tail, np.float64)
        self._check(self.call(x.ctypes.data if n else None, int(x.dtype == np.float64), n, max(n, 1),
                              None if tail is None else tail.ctypes.data, tail_out.ctypes.data, n_in, done, total - done,
                              y.ctypes.data if total > done else None, int(np.dtype(out) == np.float64), max(total - done, 1)))
        return y, (tail_out, n_in + n, total)

    def pieces(self, x, cuts, out=np.float64):
        """x cut at `cuts`, flush on the last piece only -> (list of the pieces' outputs, list of the states after each)."""
        state, ys, states = None, [], []
        for a, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            y, state = self.run(x[:, lo:hi], state, flush=a == len(cuts) - 2, out=out)
            ys.append(y)
            states.append(state)
        return ys, states


def sine(rate, n=6000, f=1000.0, amp=0.5):
    return amp * np.sin(2 * np.pi * f * np.arange(n) / rate)


def sine_error(y, L, M, C, rate_out=48000, f=1000.0, amp=0.5):
    """max |y - the analytic sine at rate_out| away from the ends: the first and last ceil(2C / M) + 2 outputs are left out."""
    skip = -(-(2 * C) // M) + 2
    assert y.shape[-1] > 2 * skip + 16, "too few outputs away from the ends"
    ref = amp * np.sin(2 * np.pi * f * np.arange(y.shape[-1]) / rate_out)
    return float(np.max(np.abs(y - ref)[..., skip:y.shape[-1] - skip]))
