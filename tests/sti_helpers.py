"""What the MtfBatch / STI tests share: the numpy restatement of X5 (include/friture_hip.h) in float64 or np.longdouble, with the
constants of IEC 60268-16:2011 written out a second time, seeded decaying-noise rows, and the distances.

The phase.  F t / fs reaches thousands of cycles, so it is reduced before cos and sin see it: t is split into bytes, F (53 bits)
times a byte (8 bits) times a power of two is exact in np.longdouble (64 bits), np.fmod(.., fs) is exact, and the four
remainders (each below fs) are added and reduced once more: the fractional part is exact up to one longdouble rounding, 5e-20
of a cycle.  The sums run in `real`."""
import functools
import math

import numpy as np

# the seeded decaying-noise row, what the strided cases share, and the two distances: max |got - want| and that over |want| (a
# NaN or the same infinity on both sides is at distance 0, a NaN on one side at inf)
from decay_helpers import STRIDED_ROWS, _frozen, response, strided_shape  # noqa: F401
from decay_helpers import db_distance as distance, rel_distance as relative  # noqa: F401

MOD_FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
ALPHA = {"male": (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173), "female": (0.0, 0.117, 0.223, 0.216, 0.328, 0.250, 0.194)}
BETA = {"male": (0.085, 0.078, 0.065, 0.011, 0.047, 0.095), "female": (0.0, 0.099, 0.066, 0.062, 0.025, 0.076)}
RECEPTION_DB = (46.0, 27.0, 12.0, 6.5, 7.5, 8.0, 12.0)
SPEECH_DB = {"male": (2.9, 2.9, -0.8, -6.8, -12.8, -18.8, -24.8), "female": (-math.inf, 5.3, -1.9, -9.1, -15.8, -16.7, -18.0)}
TWO_PI = 2 * np.arccos(np.longdouble(-1))
STIPA_HZ = ((1.6, 8.0), (1.0, 5.0), (0.63, 3.15), (2.0, 10.0), (1.25, 6.3), (0.8, 4.0), (2.5, 12.5))


def stipa_mask():
    mask = np.zeros((7, len(MOD_FREQS)), bool)
    for k, pair in enumerate(STIPA_HZ):
        for f in pair:
            mask[k, MOD_FREQS.index(f)] = True
    return mask


def cycles(F, t, fs):
    """The fractional part of F t / fs as np.longdouble, t integers below 2^32."""
    F, fs, t = np.longdouble(F), np.longdouble(fs), np.asarray(t, np.int64)
    r = np.zeros(t.shape, np.longdouble)
    for shift in (0, 8, 16, 24):
        piece = ((t >> shift) & 255).astype(np.longdouble) * np.longdouble(1 << shift)
        r += np.fmod(F * piece, fs)
    c = np.fmod(r, fs) / fs
    return np.where(c >= 0.5, c - 1, c)


def phasors(freqs, t, fs, real):
    """(cos, -sin) of 2 pi F t / fs, each [nf, len(t)] in `real`."""
    w = np.stack([cycles(F, t, fs) for F in freqs]).astype(real) * real(TWO_PI)
    return np.cos(w), -np.sin(w)


@functools.lru_cache(maxsize=4)
def _table(freqs, T, fs, real):
    return phasors(freqs, np.arange(T), fs, real)


def restate_mtf(x, freqs=MOD_FREQS, fs=48000, start=None, stop=None, real=np.float64):
    """(m [R, nf], energy [R]) of rows x [R, T] by the text of X5, sums in `real`; start, stop: None or integers [R]."""
    x = np.asarray(x, np.float64)                                    # a float32 sample widens exactly
    R, T = x.shape
    lo = np.zeros(R, np.int64) if start is None else np.broadcast_to(np.asarray(start, np.int64), (R,))
    hi = np.full(R, T, np.int64) if stop is None else np.broadcast_to(np.asarray(stop, np.int64), (R,))
    t = np.arange(T)
    inside = (t >= lo[:, None]) & (t < hi[:, None])
    bad = ~np.all(np.isfinite(np.where(inside, x, 0.0)), axis=1) | (lo < 0) | (lo >= hi) | (hi > T)
    e = np.where(inside & ~bad[:, None], x, 0.0).astype(real) ** 2
    c, s = _table(tuple(float(F) for F in freqs), T, fs, real)
    S0 = e.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.hypot(e @ c.T, e @ s.T) / S0[:, None]
    m[bad] = np.nan
    return m, S0


def masking_db(L):
    if L < 63:
        return 0.5 * L - 65
    if L < 67:
        return 1.8 * L - 146.9
    if L < 100:
        return 0.5 * L - 59.8
    return -10.0


def restate_sti(m, snr_db=None, level_db=None, noise_db=None, weights="male", scheme="full", real=np.float64):
    """X5's steps 1 to 4 on m [S, 7, nf] in `real`: a dict with sti [S], mti [S, 7], ti [S, 7, nf] and levels, every total level
    Ltot that the masking function was asked about."""
    m = np.asarray(m).astype(real)
    S, B, nf = m.shape
    assert B == 7 and not (snr_db is not None and level_db is not None)
    alpha, beta = (ALPHA[weights], BETA[weights]) if isinstance(weights, str) else weights
    alpha, beta = np.asarray(alpha, real), np.asarray(beta, real)
    mask = np.ones((7, nf), bool) if isinstance(scheme, str) and scheme == "full" else (stipa_mask() if isinstance(scheme, str) else np.asarray(scheme))
    assert mask.shape == (7, nf) and np.all(mask.any(axis=1))
    ten, levels = real(10), []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if snr_db is not None:
            snr = np.broadcast_to(np.asarray(snr_db, np.float64), (S, 7)).astype(real)
            m = m / (1 + ten ** (-snr / ten))[:, :, None]
        elif level_db is not None:
            L = np.broadcast_to(np.asarray(level_db, np.float64), (S, 7)).astype(real)
            I = ten ** (L / ten)
            In = np.zeros_like(I) if noise_db is None else ten ** (np.broadcast_to(np.asarray(noise_db, np.float64), (S, 7)).astype(real) / ten)
            Irt = ten ** (np.asarray(RECEPTION_DB, real) / ten)
            Iam = np.zeros_like(I)
            for s in range(S):
                for k in range(1, 7):
                    below = I[s, k - 1] + In[s, k - 1]
                    Ltot = ten * np.log10(below)
                    levels.append(float(Ltot))
                    Iam[s, k] = below * ten ** (real(masking_db(Ltot)) / ten)
            m = m * (I / (I + In + Iam + Irt))[:, :, None]
        snr_eff = ten * np.log10(m / (1 - m))
        snr_eff = np.where(m >= 1, real(15), np.where(m <= 0, real(-15), snr_eff))
        snr_eff = np.where(snr_eff > 15, real(15), np.where(snr_eff < -15, real(-15), snr_eff))       # a NaN stays
        ti = (snr_eff + 15) / 30
        mti = np.stack([ti[:, k, mask[k]].sum(axis=1) / real(mask[k].sum()) for k in range(7)], axis=1)
        sti = (alpha * mti).sum(axis=1) - (beta * np.sqrt(mti[:, :-1] * mti[:, 1:])).sum(axis=1)
        sti = np.where(sti > 1, real(1), sti)
    return {"sti": sti, "mti": mti, "ti": ti, "levels": levels}


def exponential_m(F, rt, fs, T, real=np.longdouble):
    """The closed form for e[t] = r^t, 0 <= t < T, r = 10^(-6 / (rt fs)): |(1 - z^T) / (1 - z)| (1 - r) / (1 - r^T), z = r exp(-2 pi i
    F / fs).  z^T is formed from r^T and the reduced phase F T / fs."""
    r = real(10) ** (real(-6) / (real(rt) * real(fs)))
    w1, wT = (real(TWO_PI * cycles(F, np.array([t]), fs)[0]) for t in (1, T))
    zr, zi = r * np.cos(w1), -r * np.sin(w1)                         # the complex arithmetic is written out in `real`
    rT = r ** real(T)
    zTr, zTi = rT * np.cos(wT), -rT * np.sin(wT)
    return np.hypot(1 - zTr, zTi) / np.hypot(1 - zr, zi) * (1 - r) / (1 - rT)


def two_sample_m(F, a, g, fs):
    """|1 + g^2 exp(-2 pi i F a / fs)| / (1 + g^2) in longdouble: two samples `a` apart with the amplitudes 1 and g."""
    w = TWO_PI * cycles(F, np.array([a]), fs)[0]
    g2 = np.longdouble(g) ** 2
    return np.hypot(1 + g2 * np.cos(w), g2 * np.sin(w)) / (1 + g2)


def compare(res, ref, label, m_bar=1e-10, energy_bar=1e-10):
    """Prints the distances of an MtfResult (numpy fields) from the reference (m, energy), then asserts the bars: absolute on m,
    relative on energy."""
    dm, de = distance(res.m, ref[0]), relative(res.energy, ref[1])
    line = f"{label}: m {dm:.3g} (bar {m_bar:g}), energy {de:.3g} relative (bar {energy_bar:g})"
    print(line)
    assert dm <= m_bar and de <= energy_bar, line


# ---- the cases of test_sti_edges_gpu.py, proven on the reference alone by test_sti_edges_cpu.py ----------------------------------

TILE = 4096                                 # sti.TILE
LEADS = (0, TILE - 1, TILE)
EDGE_T = 2 * TILE + 3
OFF_DEFAULT = ((44100, (0.63, 3.15, 12.5, 997.0, 22049.5)), (100, (0.63, 7.3, 49.9)), (96000, (0.001, 1.0, 47999.0)),
               (22050.5, (0.63, 3.0, 10000.25)), (48000, MOD_FREQS[-9:]))
STRIDED_T, STRIDED_LEADS = strided_shape(TILE)


def seam_rows(T, rows, f32):
    """[rows, T] with the lead-ins 0, TILE - 1, TILE in turn and decays that fall 60 dB over what the lead-in leaves."""
    return _frozen(np.stack([response(T, (T - LEADS[i % 3]) / 48000, 1000 * T + i, LEADS[i % 3], dtype=np.float32 if f32 else np.float64)
                             for i in range(rows)]))


@functools.lru_cache(maxsize=None)
def off_default_case(fs, freqs, f32):
    """(x [3, EDGE_T], the longdouble reference at that fs and those frequencies): the lead-ins 0, TILE - 1, TILE."""
    x = np.stack([response(EDGE_T, (EDGE_T - lead) / 48000, 7000 + (100 if f32 else 0) + i, lead, dtype=np.float32 if f32 else np.float64)
                  for i, lead in enumerate(LEADS)])
    return _frozen(x), restate_mtf(x, freqs, fs, real=np.longdouble)


@functools.lru_cache(maxsize=None)
def strided_case():
    """(the probes [4, 66 TILE + 5] float32, start = their lead-ins, the longdouble reference over [start, T) at the defaults):
    live spans of 67 and 66 tiles."""
    T = STRIDED_T
    x = np.stack([response(T, 2 * (T - lead) / 48000, 9100 + i, lead, dtype=np.float32) for i, lead in enumerate(STRIDED_LEADS)])
    start = np.array(STRIDED_LEADS, np.int64)
    return _frozen(x), _frozen(start), restate_mtf(x, start=start, real=np.longdouble)


@functools.lru_cache(maxsize=None)
def live_span_case():
    """(x [6, STRIDED_T], start, stop, the reference): probe rows over intervals of exactly 64 and 65 live tiles, from tile 0 and
    from tile 1, from a tile's first sample and from inside it."""
    probes, _, _ = strided_case()
    pairs = [(2, TILE, 65 * TILE), (2, TILE, 65 * TILE + 1), (0, 0, 64 * TILE), (0, 0, 64 * TILE + 1), (3, 3, 64 * TILE - 5),
             (1, TILE + 7, 65 * TILE + 9)]
    x = np.stack([probes[i] for i, _, _ in pairs])
    start, stop = (np.array([p[k] for p in pairs], np.int64) for k in (1, 2))
    return _frozen(x), _frozen(start), _frozen(stop), restate_mtf(x, start=start, stop=stop, real=np.longdouble)
