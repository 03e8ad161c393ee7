"""The numpy restatement of X9 (include/friture_hip.h): the fundamental, the harmonics and the residual of tone recordings,
in float64 or in np.longdouble (numpy transforms longdouble natively: the yardstick of the GPU tests), the seeded cases of the
tests and their distances.  Host only."""
import functools
import math

import numpy as np

LD = np.longdouble
FS = 48000.0


def settings_bins(N, L, band=None, f0=None, fs=FS, streams=1):
    """(ka, kb, klo [n], khi [n]) of X9's settings, n = 1 or the number of f0 values."""
    ka, kb = L + 1, N // 2
    if band is not None:
        ka, kb = max(ka, int(math.ceil(band[0] * N / fs))), min(kb, int(math.floor(band[1] * N / fs)))
    klo, khi = np.array([ka + L]), np.array([kb - L])
    if f0 is not None:
        c = np.rint(np.atleast_1d(np.asarray(f0, np.float64)) * N / fs).astype(np.int64)
        klo, khi = np.maximum(klo, c - L), np.minimum(khi, c + L)
    return ka, kb, klo, khi


def spectrum(frame, w, real=np.float64):
    """Q [N/2 + 1] of one frame [N] of float64 samples."""
    N = len(w)
    X = np.fft.rfft(np.asarray(frame, real) * np.asarray(w, real))
    c = np.full(N // 2 + 1, 2, real)
    c[0] = c[-1] = 1
    wsum = real(0)
    for v in np.asarray(w, real):
        wsum = wsum + v * v
    return c * (X.real * X.real + X.imag * X.imag) / (real(N) * wsum)


def fold(values, real):
    """The left fold from 0 of values in their order."""
    acc = real(0)
    for v in values:
        acc = acc + v
    return acc


def lobes(Q, c1, L, H, kb):
    """(P1, kappa, c [H] (c[0] = c1; -1: absent), spans [H] of (lo, hi) or None) of a frame's Q with its arg-max c1."""
    real = Q.dtype.type
    P1, num = real(0), real(0)
    for k in range(c1 - L, c1 + L + 1):
        P1 = P1 + Q[k]
        num = num + real(k) * Q[k]
    kappa = num / P1
    k64 = np.float64(kappa)                      # c_h is made from kappa as a double
    c, spans = [c1], [(c1 - L, c1 + L)]
    for h in range(2, H + 1):
        ch = int(np.rint(np.float64(h) * k64))
        cp = c1 if h == 2 else int(np.rint(np.float64(h - 1) * k64))
        if ch + L <= kb:
            c.append(ch)
            spans.append((max(ch - L, cp + L + 1), ch + L))
        else:
            c.append(-1)
            spans.append(None)
    return P1, kappa, c, spans


def lobe_sums(Q, spans):
    """P_2 .. P_H of a frame (NaN: absent) from the spans of lobes()."""
    real = Q.dtype.type
    return [real(np.nan) if sp is None else fold(Q[sp[0]:sp[1] + 1], real) for sp in spans[1:]]


def residual(Q, spans, ka, kb):
    """R of a frame in X9's order: thread i of N/16 takes the bins i + j N/16, j = 0 .. 7 (thread 0 then N/2), a bin outside the
    band or inside a lobe counts as 0; a balanced tree over each 64 consecutive threads (32 for N = 512); the groups in order."""
    real = Q.dtype.type
    M = len(Q) - 1
    Z = Q.copy()
    Z[:ka] = 0
    Z[kb + 1:] = 0
    for sp in spans:
        if sp is not None:
            Z[sp[0]:sp[1] + 1] = 0
    tpf = M // 8
    part = np.zeros(tpf, real)
    for j in range(8):
        part = part + Z[j * tpf:(j + 1) * tpf]
    part[0] = part[0] + Z[M]
    r = part.reshape(-1, min(tpf, 64))
    while r.shape[1] > 1:
        r = r[:, 0::2] + r[:, 1::2]
    return fold(r[:, 0], real)


def restate(x, N, hop, w, L, H, ka, kb, klo, khi, gate=0.0, real=np.float64):
    """X9 over the rows x [S, T] (float64 values).  A dict: kappa, fund, resid [S, F], harmonics [S, F, H - 1] in `real`, peak_bin,
    valid, centres [S, F, H] (c_h; -1 absent or dead), runner_up [S, F] (the second largest Q of the search range over the
    largest), n_valid [S], totals [S, 2 + H] (the folds of kappa, P1, R, P_2 .. P_H)."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    S, T = x.shape
    F = 0 if T < N else (T - N) // hop + 1
    nan = real(np.nan)
    out = dict(kappa=np.full((S, F), nan), fund=np.full((S, F), nan), resid=np.full((S, F), nan),
               harmonics=np.full((S, F, H - 1), nan), peak_bin=np.full((S, F), -1, np.int32), valid=np.zeros((S, F), bool),
               centres=np.full((S, F, H), -1, np.int64), runner_up=np.zeros((S, F)), n_valid=np.zeros(S, np.int64),
               totals=np.zeros((S, 2 + H), real))
    for s in range(S):
        lo, hi = int(klo[s if len(klo) > 1 else 0]), int(khi[s if len(khi) > 1 else 0])
        for f in range(F):
            frame = x[s, f * hop:f * hop + N]
            if not np.all(np.isfinite(frame)):
                continue
            Q = spectrum(frame, w, real)
            seg = Q[lo:hi + 1]
            if not np.any(seg > 0):
                continue
            c1 = lo + int(np.argmax(seg))
            if len(seg) > 1:
                out["runner_up"][s, f] = float(np.sort(seg)[-2] / seg.max())
            P1, kappa, c, spans = lobes(Q, c1, L, H, kb)
            out["kappa"][s, f], out["fund"][s, f], out["peak_bin"][s, f] = kappa, P1, c1
            out["centres"][s, f] = c
            out["harmonics"][s, f] = lobe_sums(Q, spans)
            out["resid"][s, f] = residual(Q, spans, ka, kb)
            out["valid"][s, f] = not P1 < real(gate)
            if out["valid"][s, f]:
                row = [kappa, P1, out["resid"][s, f]] + [real(0) if np.isnan(v) else v for v in out["harmonics"][s, f]]
                out["totals"][s] = out["totals"][s] + np.array(row, real)
                out["n_valid"][s] += 1
    return out


POWERS = ("fund", "resid", "harmonics")


def distances(got, ref):
    """The largest |got - ref| per quantity over the entries that are numbers in ref (the NaN patterns are compared elsewhere)."""
    out = {}
    for name in ("kappa",) + POWERS + ("totals",):
        a, b = np.asarray(got[name], LD), np.asarray(ref[name], LD)
        d = np.abs(a - b)[~np.isnan(b)]
        out[name] = float(d.max()) if d.size else 0.0
    return out


def pick_fundamental(base, H, kb, L):
    """A fundamental in bins in [base, base + 1): the fraction (a multiple of 0.01) whose present multiples h kappa stay farthest
    from a half-integer."""
    best, best_d = None, -1.0
    for step in range(3, 98):
        kappa = base + step / 100.0
        d = min(abs((h * kappa) % 1.0 - 0.5) for h in range(2, H + 1) if h * kappa + L <= kb + 1)
        if d > best_d + 1e-12:
            best, best_d = kappa, d
    return best


AMPLITUDES = {2: 1e-3, 3: 1e-5, 5: 1e-4}
NOISE = 1e-8


def tone(kappa, N, T, seed, fs=FS, amplitudes=AMPLITUDES, noise=NOISE):
    """A unit sine at bin kappa of an N-point frame with the harmonics `amplitudes` at distinct phases and white noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    x = np.sin(2 * np.pi * kappa / N * t + 0.3)
    for h, a in amplitudes.items():
        x = x + a * np.sin(2 * np.pi * h * kappa / N * t + 0.7 * h)
    return x + noise * rng.standard_normal(T)


@functools.lru_cache(maxsize=None)
def standard_case(N, hop, frames, streams, L=8, H=10, beta=20.0, dtype="float64"):
    """(x [streams, T], settings dict, ref64, refld): the recording of the parity tests, T a little more than `frames` frames,
    and the float64 and longdouble restatements of it (on the float32 values for dtype float32).  Asserts on its own reference
    the conditioning that makes the integer outputs meaningful."""
    T = N + (frames - 1) * hop + min(hop, N) // 3
    ka, kb, klo, khi = settings_bins(N, L)
    x = np.stack([tone(pick_fundamental(2 * L + 3 + 4 + 7 * s, H, kb, L), N, T, 100 * N + s) for s in range(streams)])
    x = x.astype(dtype)
    w = np.kaiser(N, beta)
    args = (x.astype(np.float64), N, hop, w, L, H, ka, kb, klo, khi)
    r64, rld = restate(*args, real=np.float64), restate(*args, real=LD)
    check_conditioning(r64, rld, L)
    x.setflags(write=False)
    return x, dict(fft_size=N, hop=hop, window=("kaiser", beta), lobe=L, harmonics=H), r64, rld


def check_conditioning(r64, rld, L):
    for name in ("peak_bin", "centres", "valid", "n_valid"):
        assert np.array_equal(r64[name], rld[name]), name
    assert np.all(r64["peak_bin"][r64["valid"]] >= 2 * L + 3)
    kappa = np.asarray(rld["kappa"], np.float64)
    for h in range(2, rld["centres"].shape[-1] + 1):
        present = rld["centres"][..., h - 1] >= 0
        assert np.all(np.abs((h * kappa[present]) % 1.0 - 0.5) >= 0.05), h
    assert np.all(rld["runner_up"][rld["peak_bin"] >= 0] <= 1 - 1e-6)


def largest(d, axis):
    """The largest entry of d along `axis` that is a number (0 where there is none), axes kept."""
    return np.max(np.where(np.isnan(d), 0, d), axis=axis, keepdims=True, initial=0).astype(np.float64)


def power_bars(r64, rld):
    """The bar on each power of a parity case: the larger of 64 times the float64 restatement's own distance from the longdouble
    one for that quantity and 1e-13 sqrt(P P_total), the scale of a transform rounding error against the loudest line.  A
    quantity is kappa, P1, R, each order's P_h and each column of the totals on its own: the own distance is the largest over
    the streams and frames of that quantity alone, so a quiet order is not measured with a loud one's error.  On kappa and its
    total the second term is 1e-10 bins per frame.  A dict of arrays that broadcast to the quantities (totals: [S, 2 + H])."""
    own = {k: np.abs(np.asarray(r64[k], LD) - rld[k]) for k in ("kappa",) + POWERS + ("totals",)}
    harm = np.nan_to_num(np.asarray(rld["harmonics"], np.float64))
    total = np.nan_to_num(np.asarray(rld["fund"], np.float64) + np.asarray(rld["resid"], np.float64)) + harm.sum(-1)
    bars = {"kappa": np.maximum(64 * largest(own["kappa"], None), 1e-10)}
    for k in POWERS:
        P = np.nan_to_num(np.asarray(rld[k], np.float64))
        tot = total[..., None] if P.ndim == 3 else total
        bars[k] = np.maximum(64 * largest(own[k], (0, 1)), 1e-13 * np.sqrt(P * tot))
    n = np.maximum(rld["n_valid"], 1).astype(np.float64)
    sums = np.asarray(rld["totals"], np.float64)
    e = largest(own["totals"], 0)
    tbar = np.maximum(64 * e, 1e-13 * np.sqrt(np.abs(sums) * sums[:, 1:].sum(-1, keepdims=True)))
    tbar[:, 0] = np.maximum(64 * e[0, 0], 1e-10 * n)
    bars["totals"] = tbar
    return bars


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def result_arrays(tb, res):
    """A ToneResult of the ToneBatch tb (numpy or CUDA, with or without the stream axis) as the restatement's dict of host arrays:
    kappa = freq N / fs (two roundings, far below its bar), totals and n_valid from the state."""
    two = lambda a, nd: a[None] if a.ndim < nd else a
    out = dict(fund=two(host(res.fund), 2), resid=two(host(res.resid), 2), harmonics=two(host(res.harmonics), 3),
               peak_bin=two(host(res.peak_bin), 2), valid=two(host(res.valid), 2), freq=two(host(res.freq), 2))
    out["kappa"] = out["freq"] / (tb.fs / tb.fft_size)
    totals = host(tb.state_parts(res.state)["totals"])
    out["totals"], out["n_valid"] = totals[:, :-1], totals[:, -1].astype(np.int64)
    return out


def same_bits(a, b):
    """Are two results (fields, totals and state) bit-identical?  The names of the fields that differ."""
    bad = []
    for name in ("freq", "fund", "resid", "harmonics", "peak_bin", "valid"):
        x, y = host(getattr(a, name)), host(getattr(b, name))
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(name)
    for name in ("n_valid", "freq", "fund", "resid", "harmonics"):
        x, y = host(getattr(a.total, name)), host(getattr(b.total, name))
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append("total." + name)
    sa, sb = a.state, b.state
    if host(sa.data).tobytes() != host(sb.data).tobytes() or tuple(sa[1:4]) != tuple(sb[1:4]):
        bad.append("state")
    return bad
